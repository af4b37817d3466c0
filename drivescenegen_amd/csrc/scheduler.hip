// Noise-scheduler elementwise kernels for gfx950 (HBM-bound streaming, float4 per lane).
//
// Replaces the tensor arithmetic of diffusers' DDPMScheduler.add_noise / .step and
// DDIMScheduler.step (reference call sites: DriveSceneGen/pipeline/training_pipeline.py:80
// `noise_scheduler.add_noise`, and the DDPMPipeline loop behind training_pipeline.py:26-32 and
// DriveSceneGen/scripts/generation.py:14-20; formulas SURVEY.md App. A.3 / A.3b / A.4), and adds the samplers diffusers ships
// next to them: RePaint, DPM-Solver++ multistep, dynamic thresholding, and the sample- / v-prediction forms of the DDPM / DDIM
// step with the training target that goes with them.
// Every expression is evaluated with individually rounded fp32 operations in the reference's
// order (fma contraction disabled for this file, IEEE division), so results are bit-identical to torch-CPU.
//
// The file reads: per-element formulas (each operation order stated ONCE) -> the training / headline kernels (add_noise, philox,
// ddpm_step, ddim_step: one loop each, untouched by the sampler features) -> the quad skeleton ("one lane owns four consecutive
// elements") and the sampler kernels built on it (RePaint, DPM-Solver++, the prediction-type step, the training target, the
// thresholded step) -> the thresholding quantile -> postprocess -> host helpers -> entry points.
#include <type_traits>

#include "dsg_common.h"

// HIP's __fmul_rn/__fadd_rn are plain operators (contractible); forbid fma contraction for this TU instead.
#pragma clang fp contract(off)

namespace dsg {

__device__ __forceinline__ float clampf(float v, float lo, float hi) { return fminf(fmaxf(v, lo), hi); }

// ---------------------------------------------------------------------------------------------------------------
// The per-element formulas.  Every kernel below that needs one calls it here, so each operation order exists once.
// a*x + b*z: two multiplies, one add (add_noise; RePaint's undo and its known / unknown blend)
__device__ __forceinline__ float axpby(float a, float x, float b, float z) {
  return __fadd_rn(__fmul_rn(a, x), __fmul_rn(b, z));
}

// r + c*z: one more term of a sum taken left to right (a noise term; DPM-Solver's higher-order terms)
__device__ __forceinline__ float add_scaled(float r, float c, float z) { return __fadd_rn(r, __fmul_rn(c, z)); }

// the data prediction p0 = (x - sb*e) / sa, clamped to +-clip when clip > 0
__device__ __forceinline__ float pred_x0(float x, float e, float sb, float sa, float clip) {
  float v = __fdiv_rn(__fsub_rn(x, __fmul_rn(sb, e)), sa);
  if (clip > 0.f) v = clampf(v, -clip, clip);
  return v;
}

// p0 clamped to +-s and divided by s (IEEE division): the thresholded data prediction
__device__ __forceinline__ float thr_x0(float x, float e, float sb, float sa, float s) {
  return __fdiv_rn(clampf(pred_x0(x, e, sb, sa, 0.f), -s, s), s);
}

// DDPM: prev = c0*p0 + ct*x, then [+ sigma*z] where the step has a noise term
__device__ __forceinline__ float ddpm_combine(float p0, float x, float c0, float ct) { return axpby(c0, p0, ct, x); }
__device__ __forceinline__ float ddpm_add_noise(float r, float sigma, float z) { return add_scaled(r, sigma, z); }

// DDIM: prev = sap*p0 + dc*e
__device__ __forceinline__ float ddim_combine(float p0, float e, float sap, float dc) { return axpby(sap, p0, dc, e); }

// a*x - b*z: two multiplies, one subtract (the data prediction of a v-predicting network; the velocity target)
__device__ __forceinline__ float axmby(float a, float x, float b, float z) {
  return __fsub_rn(__fmul_rn(a, x), __fmul_rn(b, z));
}

// What the network's output m stands for (DSG_PRED_*, include/dsg.h) decides how a step gets its data prediction p0 and its
// noise prediction pe:
//   epsilon   p0 = pred_x0(x, m)            pe = m
//   sample    p0 = m                        pe = (x - sa*m) / sb        (sb == 0: IEEE division by zero, as diffusers at abar = 1)
//   v         p0 = sa*x - sb*m              pe = sa*m + sb*x
// p0 is clamped to +-clip when clip > 0; pe is taken from the UNCLAMPED inputs and never recomputed from the clamped p0
// (diffusers' use_clipped_model_output=False, the only mode).
template <int PRED>
__device__ __forceinline__ float pred_p0(float x, float m, float sb, float sa, float clip) {
  if (PRED == DSG_PRED_EPSILON) return pred_x0(x, m, sb, sa, clip);
  float v = PRED == DSG_PRED_SAMPLE ? m : axmby(sa, x, sb, m);
  if (clip > 0.f) v = clampf(v, -clip, clip);
  return v;
}
template <int PRED>
__device__ __forceinline__ float pred_eps(float x, float m, float sb, float sa) {
  if (PRED == DSG_PRED_EPSILON) return m;
  if (PRED == DSG_PRED_SAMPLE) return __fdiv_rn(__fsub_rn(x, __fmul_rn(sa, m)), sb);
  // axpby(sa, m, sb, x), with one product pinned in a register of its own (as in repaint_elem below: hipcc otherwise pairs the
  // four products of p0 and pe into v_pk_mul_f32 and sums a pair with v_pk_add_f32 ... op_sel:[0,1], the form
  // tests/test_isa_policy.py bans; same arithmetic, same rounding)
  float am = __fmul_rn(sa, m);
  asm volatile("" : "+v"(am));
  return __fadd_rn(am, __fmul_rn(sb, x));
}

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
    r.x = axpby(a, x.x, b, e.x);
    r.y = axpby(a, x.y, b, e.y);
    r.z = axpby(a, x.z, b, e.z);
    r.w = axpby(a, x.w, b, e.w);
    *reinterpret_cast<float4*>(out + base + i0) = r;
  } else {
    for (int k = 0; k < 4 && i0 + k < per; ++k) out[base + i0 + k] = axpby(a, x0[base + i0 + k], b, nz[base + i0 + k]);
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
        q.x = axpby(a, x.x, b, z[0]);
        q.y = axpby(a, x.y, b, z[1]);
        q.z = axpby(a, x.z, b, z[2]);
        q.w = axpby(a, x.w, b, z[3]);
        *reinterpret_cast<float4*>(noisy + e) = q;
      }
    } else {
      for (int k = 0; k < 4 && e + k < numel; ++k) {
        o[e + k] = z[k];
        if (MODE == 2) {
          const int64_t n = (e + k) / per;
          noisy[e + k] = axpby(sa[n], x0[e + k], sb[n], z[k]);
        }
      }
    }
  }
}

__global__ __launch_bounds__(256) void ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                        const float* __restrict__ nz, float* __restrict__ prev,
                                                        int64_t numel, float sb, float sa, float clip, float c0,
                                                        float ct, float sigma) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const float xv = x[i];
    const float p0 = pred_x0(xv, eps[i], sb, sa, clip);
    float r = ddpm_combine(p0, xv, c0, ct);
    if (nz) r = ddpm_add_noise(r, sigma, nz[i]);
    prev[i] = r;
  }
}

__global__ __launch_bounds__(256) void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                        float* __restrict__ prev, int64_t numel, float sb, float sa,
                                                        float clip, float sap, float dc) {
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < numel; i += stride) {
    const float e = eps[i];
    prev[i] = ddim_combine(pred_x0(x[i], e, sb, sa, clip), e, sap, dc);
  }
}

// ---------------------------------------------------------------------------------------------------------------
// The quad skeleton of the sampler kernels (repaint_step, repaint_undo, dpmsolver_step, thr_step).  One lane owns one QUAD:
// the 4 consecutive elements [4q, 4q + 4) of the flat tensor, which are also one Philox block (the mapping above), so a step's
// noise can be made where it is consumed.  A kernel is
//   for_each_quad(numel, [&](q, e) { vec = quad_is_vec<VEC>(e, numel); load4 ...; noise4<NOISE> ...; arithmetic; store4 ...; })
// ONE vector rule for all of them: a launch is VEC when the host found every pointer it touches 16-byte aligned; inside a VEC
// launch a WHOLE quad (e + 4 <= numel) moves as one dwordx4 per stream; the last numel % 4 elements, and everything in a launch
// that is not VEC, take the per-element path.  Elements of a quad past numel are loaded as 0, computed and never stored.
enum { NOISE_NONE = 0, NOISE_READ = 1, NOISE_PHILOX = 2 };     // no noise term | read from `nz` | this lane's Philox block

struct philox_words {                                          // (seed, offset) as the kernels take them
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
  static philox_words of(uint64_t seed, uint64_t offset) {
    return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
  }
};

template <class F>
__device__ __forceinline__ void for_each_quad(int64_t numel, F&& body) {
  const int64_t quads = (numel + 3) >> 2;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < quads; q += stride) body(q, q << 2);
}

template <bool VEC>
__device__ __forceinline__ bool quad_is_vec(int64_t e, int64_t numel) { return VEC && e + 4 <= numel; }

__device__ __forceinline__ void load4(const float* __restrict__ p, int64_t e, int64_t numel, bool vec, float (&v)[4]) {
  if (vec) {
    const float4 t = *reinterpret_cast<const float4*>(p + e);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    for (int k = 0; k < 4; ++k) v[k] = e + k < numel ? p[e + k] : 0.f;
  }
}

__device__ __forceinline__ void store4(float* __restrict__ p, int64_t e, int64_t numel, bool vec, const float (&v)[4]) {
  if (vec) {
    *reinterpret_cast<float4*>(p + e) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    for (int k = 0; k < 4 && e + k < numel; ++k) p[e + k] = v[k];
  }
}

// the noise of quad q; echoed to `noise_out` when the caller wants the tensor the step used
template <int NOISE>
__device__ __forceinline__ void noise4(const float* __restrict__ nz, float* __restrict__ noise_out, int64_t q, int64_t numel,
                                       bool vec, const philox_words& w, float (&z)[4]) {
  if (NOISE == NOISE_NONE) {
    z[0] = z[1] = z[2] = z[3] = 0.f;
    return;
  }
  if (NOISE == NOISE_READ) {
    load4(nz, q << 2, numel, vec, z);
  } else {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)((uint64_t)q >> 32), w.off_lo, w.off_hi, w.seed_lo, w.seed_hi, r);
    box_muller(r[0], r[1], z[0], z[1]);
    box_muller(r[2], r[3], z[2], z[3]);
  }
  if (noise_out) store4(noise_out, q << 2, numel, vec, z);
}

// Per-sample values (a [numel / per] table: the thresholding scales, add_noise's coefficients) of the quad from flat index e on:
// one division when its elements share a sample (then the quad is whole).  tbl is read at index < numel / per only: an element
// past numel gets `past`.
__device__ __forceinline__ void per_sample4(const float* __restrict__ tbl, int64_t e, int64_t numel, int64_t per, float past,
                                            float (&s)[4]) {
  const int64_t n = e / per, rem = e - n * per;
  if (rem + 4 <= per) {
    s[0] = s[1] = s[2] = s[3] = tbl[n];
  } else {                                          // the quad crosses into the next sample(s), or past the end
    for (int j = 0; j < 4; ++j) s[j] = e + j < numel ? tbl[(e + j) / per] : past;
  }
}

// ---------------------------------------------------------------------------------------------------------------
// RePaint (Lugmayr et al., CVPR 2022, Algorithm 1; diffusers' RePaintScheduler.step / .undo_step): scene completion with an
// unconditional network.  One pass per reverse step, per element and in THIS order (include/dsg.h states it as the contract):
//   p0      = (x - sb*e) / sa, clamped to +-clip when clip > 0                 (pred_x0)
//   unknown = sap*p0 + dc*e     [+ std*z  when add_std]                        (ddim_combine, add_scaled)
//   known   = sap*orig + sbp*z
//   prev    = m*known + (1 - m)*unknown
// z is ONE noise value per element, used in both places (NOISE_READ: device memory or a pinned host buffer; NOISE_PHILOX).
// `orig` / `m` are addressed through their batch / channel strides (0 = broadcast).
struct repaint_geom {
  int64_t numel, chw, hw;
  int64_t orig_sn;          // 0 (one original for the batch) or chw
  int64_t m_sn, m_sc;       // mask strides over n and c: 0 where its extent is 1
  // where flat element i of the sample finds its original and its mask weight
  __device__ __forceinline__ void locate(int64_t i, int64_t& io, int64_t& im) const {
    const int64_t n = i / chw, rem = i - n * chw;
    const int64_t ch = rem / hw, p = rem - ch * hw;
    io = n * orig_sn + rem;
    im = n * m_sn + ch * m_sc + p;
  }
};

__device__ __forceinline__ float repaint_elem(float x, float e, float o, float m, float z, float sb, float sa, float clip,
                                              float sap, float dc, float sd, float sbp, bool add_std) {
  float unknown = ddim_combine(pred_x0(x, e, sb, sa, clip), e, sap, dc);
  if (add_std) unknown = add_scaled(unknown, sd, z);
  // (the empty asm pins this product in a register of its own: hipcc otherwise pairs it with sbp*z into v_pk_mul_f32 and sums
  //  the pair with v_pk_add_f32 ... op_sel:[0,1], the form tests/test_isa_policy.py bans; same arithmetic, same rounding)
  float ko = __fmul_rn(sap, o);
  asm volatile("" : "+v"(ko));
  const float known = add_scaled(ko, sbp, z);
  return axpby(m, known, __fsub_rn(1.0f, m), unknown);
}

template <int NOISE, bool VEC>
__global__ __launch_bounds__(256) void repaint_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                           const float* __restrict__ orig, const float* __restrict__ mask,
                                                           const float* __restrict__ nz, float* __restrict__ prev,
                                                           float* __restrict__ noise_out, repaint_geom g, float sb, float sa,
                                                           float clip, float sap, float dc, float sd, float sbp, int add_std,
                                                           philox_words w) {
  const bool sdz = add_std != 0;
  for_each_quad(g.numel, [&](int64_t q, int64_t e) {
    const bool vec = quad_is_vec<VEC>(e, g.numel);
    float xv[4], ev[4], ov[4], mv[4], z[4], r[4];
    load4(x, e, g.numel, vec, xv);
    load4(eps, e, g.numel, vec, ev);
    noise4<NOISE>(nz, noise_out, q, g.numel, vec, w, z);
    if (vec) {                                    // (a VEC launch has hw % 4 == 0: the quad lies in one (n, c) plane)
      int64_t io, im;
      g.locate(e, io, im);
      load4(orig, io, io + 4, true, ov);
      load4(mask, im, im + 4, true, mv);
    } else {
      for (int k = 0; k < 4; ++k) {
        int64_t io = 0, im = 0;
        const bool in = e + k < g.numel;
        if (in) g.locate(e + k, io, im);
        ov[k] = in ? orig[io] : 0.f;
        mv[k] = in ? mask[im] : 0.f;
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = repaint_elem(xv[k], ev[k], ov[k], mv[k], z[k], sb, sa, clip, sap, dc, sd, sbp, sdz);
    store4(prev, e, g.numel, vec, r);
  });
}

// RePaint's jump back in time (one forward-diffusion step): out = ck*x + cz*z, z as above
template <int NOISE, bool VEC>
__global__ __launch_bounds__(256) void repaint_undo_kernel(const float* __restrict__ x, const float* __restrict__ nz,
                                                           float* __restrict__ out, int64_t numel, float ck, float cz,
                                                           philox_words w) {
  for_each_quad(numel, [&](int64_t q, int64_t e) {
    const bool vec = quad_is_vec<VEC>(e, numel);
    float xv[4], z[4], r[4];
    load4(x, e, numel, vec, xv);
    noise4<NOISE>(nz, nullptr, q, numel, vec, w, z);
#pragma unroll
    for (int k = 0; k < 4; ++k) r[k] = axpby(ck, xv[k], cz, z[k]);
    store4(out, e, numel, vec, r);
  });
}

// ---------------------------------------------------------------------------------------------------------------
// DPM-Solver++ multistep (Lu et al., 2022; diffusers' DPMSolverMultistepScheduler.step): the data-prediction form of the
// diffusion ODE's exponential integrator, orders 1-3, and its SDE variant.  One pass per step, per element and in THIS order
// (include/dsg.h states it as the contract):
//   m0   = (x - sigma_s*e) / alpha_s                      -> m0_out (the history entry this step adds)
//   D10  = inv_r0*(m0 - m1)                               ORDER >= 2
//   D11  = inv_r1*(m1 - m2);  dd = D10 - D11;  D1 = D10 + q*dd;  D2 = p*dd        ORDER == 3 (D1 = D10 at order 2)
//   prev = kx*x + c0*m0  [+ c1*D1]  [+ c2*D2]  [+ cn*z]   summed left to right
// The host passes signed coefficients.
struct dpm_coef {
  float sigma_s, alpha_s, inv_r0, inv_r1, q, p, kx, c0, c1, c2, cn;
};

template <int ORDER, bool NOISE>
__device__ __forceinline__ void dpm_elem(float x, float e, float m1, float m2, float z, const dpm_coef& k, float& prev,
                                         float& m0o) {
  const float m0 = pred_x0(x, e, k.sigma_s, k.alpha_s, 0.f);
  float r = axpby(k.kx, x, k.c0, m0);
  if (ORDER >= 2) {
    const float d10 = __fmul_rn(k.inv_r0, __fsub_rn(m0, m1));
    float d1 = d10;
    if (ORDER == 3) {
      const float d11 = __fmul_rn(k.inv_r1, __fsub_rn(m1, m2));
      const float dd = __fsub_rn(d10, d11);
      d1 = add_scaled(d10, k.q, dd);
      r = add_scaled(r, k.c1, d1);
      r = add_scaled(r, k.c2, __fmul_rn(k.p, dd));
    } else {
      r = add_scaled(r, k.c1, d1);
    }
  }
  if (NOISE) r = add_scaled(r, k.cn, z);
  prev = r;
  m0o = m0;
}

template <int ORDER, int NOISE, bool VEC>
__global__ __launch_bounds__(256) void dpmsolver_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                             const float* __restrict__ m1, const float* __restrict__ m2,
                                                             const float* __restrict__ nz, float* __restrict__ prev,
                                                             float* __restrict__ m0_out, float* __restrict__ noise_out,
                                                             int64_t numel, dpm_coef k, philox_words w) {
  for_each_quad(numel, [&](int64_t q, int64_t e) {
    const bool vec = quad_is_vec<VEC>(e, numel);
    float xv[4], ev[4], av[4] = {0.f, 0.f, 0.f, 0.f}, bv[4] = {0.f, 0.f, 0.f, 0.f}, z[4], r[4], m[4];
    load4(x, e, numel, vec, xv);
    load4(eps, e, numel, vec, ev);
    if (ORDER >= 2) load4(m1, e, numel, vec, av);
    if (ORDER == 3) load4(m2, e, numel, vec, bv);
    noise4<NOISE>(nz, noise_out, q, numel, vec, w, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) dpm_elem<ORDER, NOISE != NOISE_NONE>(xv[j], ev[j], av[j], bv[j], z[j], k, r[j], m[j]);
    store4(prev, e, numel, vec, r);
    store4(m0_out, e, numel, vec, m);
  });
}

// ---------------------------------------------------------------------------------------------------------------
// The DDPM / DDIM step of a network that predicts epsilon, the sample or v (Salimans & Ho, "Progressive Distillation for Fast
// Sampling of Diffusion Models", 2022; diffusers' `prediction_type`).  One pass, per element (include/dsg.h states it as the
// contract): p0 = pred_p0<PRED>, then
//   MODE 0, DDPM:  prev = c0*p0 + ct*x  [+ sigma*z]      (a = c0, b = ct, c = sigma; NOISE_READ when the step has a noise term)
//   MODE 1, DDIM:  prev = sap*p0 + dc*pe                 (a = sap, b = dc; pe = pred_eps<PRED>; NOISE_NONE)
// With PRED == DSG_PRED_EPSILON these are ddpm_step_kernel's / ddim_step_kernel's bits.
template <int MODE, int PRED, int NOISE, bool VEC>
__global__ __launch_bounds__(256) void pt_step_kernel(const float* __restrict__ x, const float* __restrict__ mo,
                                                      const float* __restrict__ nz, float* __restrict__ prev, int64_t numel,
                                                      float sb, float sa, float clip, float a, float b, float c) {
  static_assert(NOISE != NOISE_PHILOX && (MODE == 0 || NOISE == NOISE_NONE), "these steps read their noise or have none");
  for_each_quad(numel, [&](int64_t q, int64_t e) {
    const bool vec = quad_is_vec<VEC>(e, numel);
    float xv[4], mv[4], z[4], r[4];
    load4(x, e, numel, vec, xv);
    load4(mo, e, numel, vec, mv);
    noise4<NOISE>(nz, nullptr, q, numel, vec, philox_words{}, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p0 = pred_p0<PRED>(xv[j], mv[j], sb, sa, clip);
      r[j] = MODE == 1 ? ddim_combine(p0, pred_eps<PRED>(xv[j], mv[j], sb, sa), a, b) : ddpm_combine(p0, xv[j], a, b);
      if (NOISE != NOISE_NONE) r[j] = ddpm_add_noise(r[j], c, z[j]);
    }
    store4(prev, e, numel, vec, r);
  });
}

// The training step's x_t and its velocity target in one pass over (x0, z):  noisy = sa[n]*x0 + sb[n]*z (add_noise_kernel's
// bits), target = sa[n]*z - sb[n]*x0, n the sample of the ELEMENT (a quad may straddle two samples when per % 4 != 0).
// z: NOISE_READ, or NOISE_PHILOX -- the stream of philox_kernel.  Either output may be NULL (the same in every lane).
template <int NOISE, bool VEC>
__global__ __launch_bounds__(256) void noise_target_kernel(const float* __restrict__ x0, const float* __restrict__ nz,
                                                           const float* __restrict__ sa, const float* __restrict__ sb,
                                                           float* __restrict__ noisy, float* __restrict__ target, int64_t numel,
                                                           int64_t per, philox_words w) {
  static_assert(NOISE != NOISE_NONE, "the forward process has a noise term");
  for_each_quad(numel, [&](int64_t q, int64_t e) {
    const bool vec = quad_is_vec<VEC>(e, numel);
    float xv[4], z[4], a[4], b[4], r[4];
    load4(x0, e, numel, vec, xv);
    noise4<NOISE>(nz, nullptr, q, numel, vec, w, z);
    per_sample4(sa, e, numel, per, 0.f, a);
    per_sample4(sb, e, numel, per, 0.f, b);
    if (noisy) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = axpby(a[j], xv[j], b[j], z[j]);
      store4(noisy, e, numel, vec, r);
    }
    if (target) {
#pragma unroll
      for (int j = 0; j < 4; ++j) r[j] = axmby(a[j], z[j], b[j], xv[j]);
      store4(target, e, numel, vec, r);
    }
  });
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

// The DDPM / DDIM step with the thresholded data prediction.
// MODE 0: DDPM (ddpm_combine: a = c0, b = ct, c = sigma; NOISE_READ when the step has a noise term);  1: DDIM (ddim_combine:
// a = sap, b = dc; NOISE_NONE)
template <int MODE, int NOISE, bool VEC>
__global__ __launch_bounds__(256) void thr_step_kernel(const float* __restrict__ x, const float* __restrict__ eps,
                                                       const float* __restrict__ nz, const float* __restrict__ thr,
                                                       float* __restrict__ prev, int64_t numel, int64_t per, float sb, float sa,
                                                       float a, float b, float c) {
  static_assert(NOISE != NOISE_PHILOX && (MODE == 0 || NOISE == NOISE_NONE), "the thresholded steps read their noise or have none");
  for_each_quad(numel, [&](int64_t q, int64_t e) {
    const bool vec = quad_is_vec<VEC>(e, numel);
    float xv[4], ev[4], z[4], s[4], r[4];
    load4(x, e, numel, vec, xv);
    load4(eps, e, numel, vec, ev);
    noise4<NOISE>(nz, nullptr, q, numel, vec, philox_words{}, z);
    per_sample4(thr, e, numel, per, 1.f, s);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float p0 = thr_x0(xv[j], ev[j], sb, sa, s[j]);
      r[j] = MODE == 1 ? ddim_combine(p0, ev[j], a, b) : ddpm_combine(p0, xv[j], a, b);
      if (NOISE != NOISE_NONE) r[j] = ddpm_add_noise(r[j], c, z[j]);
    }
    store4(prev, e, numel, vec, r);
  });
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

// ---------------------------------------------------------------------------------------------------------------
// Host helpers of the entry points below.
static inline int capped_blocks(int64_t lanes, int64_t cap) {
  const int64_t b = cdiv64(lanes, 256);
  return (int)(b < 1 ? 1 : (b > cap ? cap : b));
}
// grid of a grid-stride kernel whose lane owns one ELEMENT (ddpm_step, ddim_step) / one QUAD (philox and the quad kernels)
static inline int elem_blocks(int64_t numel) { return capped_blocks(numel, 256 * 16); }
static inline int quad_blocks(int64_t numel) { return capped_blocks(cdiv64(numel, 4), 256 * 32); }

// NULL counts as aligned: a stream the launch does not touch does not keep it from being VEC
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
template <class... P>
static inline bool all_aligned16(const P*... p) { return (aligned16(p) && ...); }

// do [a, a + abytes) and [b, b + bbytes) share a byte?  (NULL overlaps nothing)
static inline bool overlaps2(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y ? y - x < abytes : x - y < bbytes;
}

// A run-time value v in [0, N) as a template argument: calls f(std::integral_constant<int, v>{}).  The one way this file picks
// a kernel instantiation: with_constant<2>(vec, [&](auto VEC) { launch kernel<decltype(VEC)::value != 0> ... }).
template <int N, class F>
static inline void with_constant(int v, F&& f) {
  if constexpr (N > 1) {
    if (v == N - 1) f(std::integral_constant<int, N - 1>{});
    else with_constant<N - 1>(v, f);
  } else {
    f(std::integral_constant<int, 0>{});
  }
}
#define DSG_CONST(c) (decltype(c)::value)

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
  hipLaunchKernelGGL(dsg::ddpm_step_kernel, dim3(dsg::elem_blocks(numel)), dim3(256), 0,
                     static_cast<hipStream_t>(stream), sample, eps, noise, prev, numel, sqrt_beta_prod_t,
                     sqrt_alpha_prod_t, clip, coef_x0, coef_xt, sigma);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_ddim_step(const float* sample, const float* eps, float* prev, int64_t numel, float sqrt_beta_prod_t,
                          float sqrt_alpha_prod_t, float clip, float sqrt_alpha_prev, float dir_coef, void* stream) {
  DSG_CHECK_ARG(sample && eps && prev, "dsg_ddim_step: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_ddim_step: numel must be positive");
  hipLaunchKernelGGL(dsg::ddim_step_kernel, dim3(dsg::elem_blocks(numel)), dim3(256), 0,
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
  dsg::with_constant<3>(mode, [&](auto MODE) {
    hipLaunchKernelGGL(dsg::postprocess_kernel<DSG_CONST(MODE)>, grid, dim3(256), 0, st, x, out, c, hw);
  });
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
template <int MODE>
static void philox_launch(const float* x0, const float* sa, const float* sb, float* noisy, void* out, int64_t numel, int64_t per,
                          uint64_t seed, uint64_t offset, void* stream) {
  const philox_words w = philox_words::of(seed, offset);
  hipLaunchKernelGGL(philox_kernel<MODE>, dim3(quad_blocks(numel)), dim3(256), 0, static_cast<hipStream_t>(stream), x0, sa, sb,
                     noisy, out, numel, per, w.seed_lo, w.seed_hi, w.off_lo, w.off_hi);
}
}  // namespace dsg

DSG_API int dsg_philox_u32(uint32_t* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(out, "dsg_philox_u32: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_philox_u32: numel must be positive");
  dsg::philox_launch<0>(nullptr, nullptr, nullptr, nullptr, out, numel, 4, seed, offset, stream);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_philox_normal(float* out, int64_t numel, uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(out, "dsg_philox_normal: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_philox_normal: numel must be positive");
  dsg::philox_launch<1>(nullptr, nullptr, nullptr, nullptr, out, numel, 4, seed, offset, stream);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_add_noise_philox(const float* x0, const float* sqrt_a, const float* sqrt_1ma, float* noisy, float* noise,
                                 int32_t n, int64_t per_sample, uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(x0 && sqrt_a && sqrt_1ma && noisy && noise, "dsg_add_noise_philox: NULL pointer");
  DSG_CHECK_ARG(n > 0 && per_sample > 0, "dsg_add_noise_philox: bad dims");
  dsg::philox_launch<2>(x0, sqrt_a, sqrt_1ma, noisy, noise, (int64_t)n * per_sample, per_sample, seed, offset, stream);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
template <int PASS>
static void thr_pass(const float* x, const float* e, uint32_t* ws, float* s, int32_t n, int64_t per, float sb, float sa,
                     uint32_t k_lo, uint32_t k_hi, float w, float max_value, bool vec, hipStream_t st) {
  // enough blocks per sample to fill the chip at any batch, never more than the sample has 1024-element chunks
  int64_t bps = cdiv64(per, 1024), cap = cdiv64(2048, n);
  if (bps > cap) bps = cap;
  const dim3 grid((unsigned)bps, (unsigned)n), block(256);
  with_constant<2>(vec, [&](auto VEC) {
    hipLaunchKernelGGL((thr_hist_kernel<PASS, DSG_CONST(VEC) != 0>), grid, block, 0, st, x, e, ws, per, sb, sa);
  });
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
  const bool vec = (per_sample & 3) == 0 && dsg::all_aligned16(sample, eps);
  const uint32_t lo = (uint32_t)k_lo, hi = (uint32_t)k_hi;
  dsg::thr_pass<1>(sample, eps, ws, s, n, per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, lo, hi, w, sample_max_value, vec, st);
  dsg::thr_pass<2>(sample, eps, ws, s, n, per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, lo, hi, w, sample_max_value, vec, st);
  dsg::thr_pass<3>(sample, eps, ws, s, n, per_sample, sqrt_beta_prod_t, sqrt_alpha_prod_t, lo, hi, w, sample_max_value, vec, st);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

namespace dsg {
// both thresholded steps: the checks, then thr_step_kernel<MODE, noise ? NOISE_READ : NOISE_NONE, every pointer aligned>
template <int MODE>
static int thr_step(const char* who, const float* sample, const float* eps, const float* noise, const float* thr, float* prev,
                    int64_t numel, int64_t per, float sb, float sa, float a, float b, float c, void* stream) {
  if (!(sample && eps && thr && prev)) return fail(DSG_ERR_INVALID_ARG, "%s: NULL pointer", who);
  if (numel <= 0) return fail(DSG_ERR_INVALID_ARG, "%s: numel must be positive", who);
  if (per <= 0 || numel % per != 0)
    return fail(DSG_ERR_INVALID_ARG, "%s: per_sample=%lld does not divide numel=%lld", who, (long long)per, (long long)numel);
  if (overlaps2(prev, (uint64_t)numel * sizeof(float), thr, (uint64_t)(numel / per) * sizeof(float)))
    return fail(DSG_ERR_INVALID_ARG, "%s: prev overlaps thr", who);
  const dim3 grid(quad_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_constant<2>(noise != nullptr, [&](auto NZ) {
    with_constant<2>(all_aligned16(sample, eps, noise, prev), [&](auto VEC) {
      // (NOISE_READ exists for the DDPM form only: MODE 1 is always called without noise)
      hipLaunchKernelGGL((thr_step_kernel<MODE, MODE == 0 ? DSG_CONST(NZ) : NOISE_NONE, DSG_CONST(VEC) != 0>), grid, block, 0, st,
                         sample, eps, noise, thr, prev, numel, per, sb, sa, a, b, c);
    });
  });
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}
}  // namespace dsg

DSG_API int dsg_ddpm_step_thr(const float* sample, const float* eps, const float* noise, const float* thr, float* prev,
                              int64_t numel, int64_t per_sample, float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float coef_x0,
                              float coef_xt, float sigma, void* stream) {
  return dsg::thr_step<0>("dsg_ddpm_step_thr", sample, eps, noise, thr, prev, numel, per_sample, sqrt_beta_prod_t,
                          sqrt_alpha_prod_t, coef_x0, coef_xt, sigma, stream);
}

DSG_API int dsg_ddim_step_thr(const float* sample, const float* eps, const float* thr, float* prev, int64_t numel,
                              int64_t per_sample, float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float sqrt_alpha_prev,
                              float dir_coef, void* stream) {
  return dsg::thr_step<1>("dsg_ddim_step_thr", sample, eps, nullptr, thr, prev, numel, per_sample, sqrt_beta_prod_t,
                          sqrt_alpha_prod_t, sqrt_alpha_prev, dir_coef, 0.f, stream);
}

namespace dsg {
// both prediction-type steps: the checks, then pt_step_kernel<MODE, pred_type, noise ? NOISE_READ : NOISE_NONE, every pointer aligned>
template <int MODE>
static int pt_step(const char* who, const float* sample, const float* model_out, const float* noise, float* prev, int64_t numel,
                   int32_t pred_type, float sb, float sa, float clip, float a, float b, float c, void* stream) {
  if (!(sample && model_out && prev)) return fail(DSG_ERR_INVALID_ARG, "%s: NULL pointer", who);
  if (numel <= 0) return fail(DSG_ERR_INVALID_ARG, "%s: numel must be positive", who);
  if (pred_type < DSG_PRED_EPSILON || pred_type > DSG_PRED_V)
    return fail(DSG_ERR_INVALID_ARG, "%s: pred_type=%d is not DSG_PRED_EPSILON, DSG_PRED_SAMPLE or DSG_PRED_V", who, pred_type);
  const uint64_t bytes = (uint64_t)numel * sizeof(float);
  const void* ins[3] = {sample, model_out, noise};
  for (int i = 0; i < 3; ++i)
    if (overlaps2(prev, bytes, ins[i], bytes)) return fail(DSG_ERR_INVALID_ARG, "%s: prev overlaps an input (input %d)", who, i);
  const dim3 grid(quad_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  with_constant<3>(pred_type, [&](auto PRED) {
    with_constant<2>(noise != nullptr, [&](auto NZ) {
      with_constant<2>(all_aligned16(sample, model_out, noise, prev), [&](auto VEC) {
        // (NOISE_READ exists for the DDPM form only: MODE 1 is always called without noise)
        hipLaunchKernelGGL((pt_step_kernel<MODE, DSG_CONST(PRED), MODE == 0 ? DSG_CONST(NZ) : NOISE_NONE, DSG_CONST(VEC) != 0>), grid,
                           block, 0, st, sample, model_out, noise, prev, numel, sb, sa, clip, a, b, c);
      });
    });
  });
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

// both training-target entries: the checks, then noise_target_kernel<noise ? NOISE_READ : NOISE_PHILOX, every pointer aligned>
static int noise_target(const char* who, const float* x0, const float* noise, const float* sa, const float* sb, float* noisy,
                        float* target, int32_t n, int64_t per, uint64_t seed, uint64_t offset, void* stream) {
  if (!(x0 && sa && sb)) return fail(DSG_ERR_INVALID_ARG, "%s: NULL pointer", who);
  if (!noisy && !target) return fail(DSG_ERR_INVALID_ARG, "%s: noisy and target are both NULL", who);
  if (n <= 0 || per <= 0) return fail(DSG_ERR_INVALID_ARG, "%s: bad dims (n=%d per_sample=%lld)", who, n, (long long)per);
  const int64_t numel = (int64_t)n * per;
  const uint64_t bytes = (uint64_t)numel * sizeof(float), tbl = (uint64_t)n * sizeof(float);
  const void* ins[4] = {x0, noise, sa, sb};
  const uint64_t in_bytes[4] = {bytes, bytes, tbl, tbl};
  float* outs[2] = {noisy, target};
  for (int o = 0; o < 2; ++o)
    for (int i = 0; i < 4; ++i)
      if (overlaps2(outs[o], bytes, ins[i], in_bytes[i]))
        return fail(DSG_ERR_INVALID_ARG, "%s: an output overlaps an input (output %d, input %d)", who, o, i);
  if (overlaps2(noisy, bytes, target, bytes)) return fail(DSG_ERR_INVALID_ARG, "%s: noisy overlaps target", who);
  const dim3 grid(quad_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const philox_words w = philox_words::of(seed, offset);
  with_constant<2>(noise == nullptr, [&](auto PHILOX) {
    with_constant<2>(all_aligned16(x0, noise, noisy, target), [&](auto VEC) {
      hipLaunchKernelGGL((noise_target_kernel<NOISE_READ + DSG_CONST(PHILOX), DSG_CONST(VEC) != 0>), grid, block, 0, st, x0, noise,
                         sa, sb, noisy, target, numel, per, w);
    });
  });
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}
}  // namespace dsg

DSG_API int dsg_ddpm_step_pt(const float* sample, const float* model_out, const float* noise, float* prev, int64_t numel,
                             int32_t pred_type, float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float clip, float coef_x0,
                             float coef_xt, float sigma, void* stream) {
  return dsg::pt_step<0>("dsg_ddpm_step_pt", sample, model_out, noise, prev, numel, pred_type, sqrt_beta_prod_t, sqrt_alpha_prod_t,
                         clip, coef_x0, coef_xt, sigma, stream);
}

DSG_API int dsg_ddim_step_pt(const float* sample, const float* model_out, float* prev, int64_t numel, int32_t pred_type,
                             float sqrt_beta_prod_t, float sqrt_alpha_prod_t, float clip, float sqrt_alpha_prev, float dir_coef,
                             void* stream) {
  return dsg::pt_step<1>("dsg_ddim_step_pt", sample, model_out, nullptr, prev, numel, pred_type, sqrt_beta_prod_t,
                         sqrt_alpha_prod_t, clip, sqrt_alpha_prev, dir_coef, 0.f, stream);
}

DSG_API int dsg_add_noise_target(const float* x0, const float* noise, const float* sqrt_a, const float* sqrt_1ma, float* noisy,
                                 float* target, int32_t n, int64_t per_sample, void* stream) {
  DSG_CHECK_ARG(noise, "dsg_add_noise_target: NULL pointer");
  return dsg::noise_target("dsg_add_noise_target", x0, noise, sqrt_a, sqrt_1ma, noisy, target, n, per_sample, 0, 0, stream);
}

DSG_API int dsg_add_noise_target_philox(const float* x0, const float* sqrt_a, const float* sqrt_1ma, float* noisy, float* target,
                                        int32_t n, int64_t per_sample, uint64_t seed, uint64_t offset, void* stream) {
  return dsg::noise_target("dsg_add_noise_target_philox", x0, nullptr, sqrt_a, sqrt_1ma, noisy, target, n, per_sample, seed,
                           offset, stream);
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
  // hw % 4 == 0 on top of the alignment, for this kernel alone: `original` and `mask` are broadcast, so their dwordx4 load
  // needs the whole quad inside ONE (n, c) plane (it also makes numel % 4 == 0: a VEC launch has no per-element tail)
  const bool vec = (g.hw & 3) == 0 &&
                   dsg::all_aligned16(a->sample, a->eps, a->original, a->mask, a->prev, a->noise, a->noise_out);
  const dim3 grid(dsg::quad_blocks(g.numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dsg::philox_words w = dsg::philox_words::of(a->seed, a->offset);
  dsg::with_constant<2>(a->noise == nullptr, [&](auto PHILOX) {
    dsg::with_constant<2>(vec, [&](auto VEC) {
      hipLaunchKernelGGL((dsg::repaint_step_kernel<dsg::NOISE_READ + DSG_CONST(PHILOX), DSG_CONST(VEC) != 0>), grid, block, 0, st,
                         a->sample, a->eps, a->original, a->mask, a->noise, a->prev, a->noise_out, g, a->sqrt_beta_prod_t,
                         a->sqrt_alpha_prod_t, a->clip, a->sqrt_alpha_prev, a->dir_coef, a->std, a->sqrt_beta_prev, a->add_std, w);
    });
  });
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_repaint_undo(const float* sample, const float* noise, float* out, int64_t numel, float ck, float cz,
                             uint64_t seed, uint64_t offset, void* stream) {
  DSG_CHECK_ARG(sample && out, "dsg_repaint_undo: NULL pointer");
  DSG_CHECK_ARG(numel > 0, "dsg_repaint_undo: numel must be positive");
  const dim3 grid(dsg::quad_blocks(numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const dsg::philox_words w = dsg::philox_words::of(seed, offset);
  dsg::with_constant<2>(noise == nullptr, [&](auto PHILOX) {
    dsg::with_constant<2>(dsg::all_aligned16(sample, out, noise), [&](auto VEC) {
      hipLaunchKernelGGL((dsg::repaint_undo_kernel<dsg::NOISE_READ + DSG_CONST(PHILOX), DSG_CONST(VEC) != 0>), grid, block, 0, st,
                         sample, noise, out, numel, ck, cz, w);
    });
  });
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_dpmsolver_step(const dsg_dpmsolver_step_args* a, void* stream) {
  DSG_CHECK_ARG(a, "dsg_dpmsolver_step: NULL args");
  DSG_CHECK_ARG(a->sample && a->eps && a->prev && a->m0_out, "dsg_dpmsolver_step: NULL pointer");
  DSG_CHECK_ARG(a->numel > 0, "dsg_dpmsolver_step: numel must be positive");
  DSG_CHECK_ARG(a->order >= 1 && a->order <= 3, "dsg_dpmsolver_step: order=%d is not 1, 2 or 3", a->order);
  DSG_CHECK_ARG(a->order < 2 || a->m1, "dsg_dpmsolver_step: order %d needs the history entry m1", a->order);
  DSG_CHECK_ARG(a->order < 3 || a->m2, "dsg_dpmsolver_step: order %d needs the history entry m2", a->order);
  // what THIS call reads and writes (a history entry above the order, or a noise pointer without add_noise, is not touched):
  // the kernels get exactly the pointers checked here
  const float* m1 = a->order >= 2 ? a->m1 : nullptr;
  const float* m2 = a->order >= 3 ? a->m2 : nullptr;
  const float* nz = a->add_noise ? a->noise : nullptr;
  float* nout = a->add_noise ? a->noise_out : nullptr;
  const uint64_t bytes = (uint64_t)a->numel * sizeof(float);
  const void* ins[5] = {a->sample, a->eps, m1, m2, nz};
  const void* outs[3] = {a->prev, a->m0_out, nout};
  for (int o = 0; o < 3; ++o) {
    for (int i = 0; i < 5; ++i)
      DSG_CHECK_ARG(!dsg::overlaps2(outs[o], bytes, ins[i], bytes),
                    "dsg_dpmsolver_step: an output overlaps an input (output %d, input %d)", o, i);
    for (int p = o + 1; p < 3; ++p)
      DSG_CHECK_ARG(!dsg::overlaps2(outs[o], bytes, outs[p], bytes), "dsg_dpmsolver_step: two outputs overlap (%d, %d)", o, p);
  }
  const bool vec = dsg::all_aligned16(a->sample, a->eps, m1, m2, nz, a->prev, a->m0_out, nout);
  const int noise = !a->add_noise ? dsg::NOISE_NONE : (nz ? dsg::NOISE_READ : dsg::NOISE_PHILOX);
  const dsg::dpm_coef k = {a->sigma_s, a->alpha_s, a->inv_r0, a->inv_r1, a->q, a->p, a->kx, a->c0, a->c1, a->c2, a->cn};
  const dsg::philox_words w = dsg::philox_words::of(a->seed, a->offset);
  const dim3 grid(dsg::quad_blocks(a->numel)), block(256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  dsg::with_constant<3>(a->order - 1, [&](auto ORDER1) {
    dsg::with_constant<3>(noise, [&](auto NZ) {
      dsg::with_constant<2>(vec, [&](auto VEC) {
        hipLaunchKernelGGL((dsg::dpmsolver_step_kernel<DSG_CONST(ORDER1) + 1, DSG_CONST(NZ), DSG_CONST(VEC) != 0>), grid, block, 0,
                           st, a->sample, a->eps, m1, m2, nz, a->prev, a->m0_out, nout, a->numel, k, w);
      });
    });
  });
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
