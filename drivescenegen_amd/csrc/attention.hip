// Self-attention core softmax(Q^T K / sqrt(d)) V for gfx950, fp32, head_dim 8..64.
//
// Replaces F.scaled_dot_product_attention inside diffusers' Attention block as instantiated by
// UNetMidBlock2D (and Attn{Down,Up}Block2D) of the UNet2DModel that DriveSceneGen builds at
// DriveSceneGen/scripts/train.py:39-57 (attention_head_dim = 8 -> 64 heads x 8 dims over 1024 tokens;
// SURVEY.md App. A.2).  0.6 % of the network's FLOPs; K = d = 8 starves an MFMA tile, so this first
// version runs the two tiny contractions on the VALU with K/V tiles broadcast from LDS and a
// chunked online softmax; each thread owns QPT query rows so a K/V LDS read is amortised QPT times.
//
// Layout: qkv [N][3C][L] is the output of the fused q/k/v projection (a 1x1 conv over [N,C,L]);
// channel = head*D + i, so a head's q/k/v are D rows of L contiguous floats.  out is [N][C][L].
#include "att_mfma8.h"
#include "tuning.h"

namespace dsg {

constexpr int ATT_LDS_FLOATS = 4096;  // per K and per V tile: 16 KiB each, keys per tile = 4096 / D
constexpr int ATT_KB = 8;    // keys per online-softmax chunk

template <int D, int QPT>
__global__ __launch_bounds__(256) void attention_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                        float* __restrict__ lse, int c, int heads, int l, float qscale) {
  constexpr int ATT_KT = ATT_LDS_FLOATS / D;
  __shared__ __attribute__((aligned(16))) float KVl[2 * ATT_KT * D];
  float* Kl = KVl;
  float* Vl = KVl + ATT_KT * D;
  const int tid = threadIdx.x;
  const int h = blockIdx.y, n = blockIdx.z;
  const float* qp = qkv + ((size_t)n * 3 * c + h * D) * l;
  const float* kp = qp + (size_t)c * l;
  const float* vp = kp + (size_t)c * l;

  float q[QPT][D], o[QPT][D], m[QPT], lsum[QPT];
  int qi[QPT];
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    qi[u] = (blockIdx.x * QPT + u) * 256 + tid;
    const int qc = min(qi[u], l - 1);
#pragma unroll
    for (int i = 0; i < D; ++i) {
      q[u][i] = qp[(size_t)i * l + qc] * qscale;
      o[u][i] = 0.f;
    }
    m[u] = -1e30f;
    lsum[u] = 0.f;
  }

  for (int j0 = 0; j0 < l; j0 += ATT_KT) {
    const int kt = min(ATT_KT, l - j0);
    __syncthreads();
    for (int e = tid; e < ATT_KT * D; e += 256) {
      const int i = e / ATT_KT, j = e - i * ATT_KT;  // coalesced global read along j
      float kv = 0.f, vv = 0.f;
      if (j < kt) {
        kv = kp[(size_t)i * l + j0 + j];
        vv = vp[(size_t)i * l + j0 + j];
      }
      Kl[j * D + i] = kv;
      Vl[j * D + i] = vv;
    }
    __syncthreads();
    const int nchunk = (kt + ATT_KB - 1) / ATT_KB;
    for (int ch = 0; ch < nchunk; ++ch) {
      const int jb = ch * ATT_KB;
      float s[QPT][ATT_KB];
#pragma unroll
      for (int jj = 0; jj < ATT_KB; ++jj) {
        float kr[D];
#pragma unroll
        for (int i4 = 0; i4 < D; i4 += 4) {
          const float4 t = *reinterpret_cast<const float4*>(&Kl[(jb + jj) * D + i4]);
          kr[i4] = t.x; kr[i4 + 1] = t.y; kr[i4 + 2] = t.z; kr[i4 + 3] = t.w;
        }
        const bool valid = (jb + jj) < kt;
#pragma unroll
        for (int u = 0; u < QPT; ++u) {
          float a = 0.f;
#pragma unroll
          for (int i = 0; i < D; ++i) a = fmaf(q[u][i], kr[i], a);
          s[u][jj] = valid ? a : -1e30f;
        }
      }
#pragma unroll
      for (int u = 0; u < QPT; ++u) {
        float mx = s[u][0];
#pragma unroll
        for (int jj = 1; jj < ATT_KB; ++jj) mx = fmaxf(mx, s[u][jj]);
        const float mn = fmaxf(m[u], mx);
        const float sc = exp2f(m[u] - mn);
        m[u] = mn;
        float ps = 0.f;
#pragma unroll
        for (int jj = 0; jj < ATT_KB; ++jj) {
          s[u][jj] = exp2f(s[u][jj] - mn);
          ps += s[u][jj];
        }
        lsum[u] = lsum[u] * sc + ps;
#pragma unroll
        for (int i = 0; i < D; ++i) o[u][i] *= sc;
      }
#pragma unroll
      for (int jj = 0; jj < ATT_KB; ++jj) {
        float vr[D];
#pragma unroll
        for (int i4 = 0; i4 < D; i4 += 4) {
          const float4 t = *reinterpret_cast<const float4*>(&Vl[(jb + jj) * D + i4]);
          vr[i4] = t.x; vr[i4 + 1] = t.y; vr[i4 + 2] = t.z; vr[i4 + 3] = t.w;
        }
#pragma unroll
        for (int u = 0; u < QPT; ++u)
#pragma unroll
          for (int i = 0; i < D; ++i) o[u][i] = fmaf(s[u][jj], vr[i], o[u][i]);
      }
    }
  }

  float* op = out + ((size_t)n * c + h * D) * l;
#pragma unroll
  for (int u = 0; u < QPT; ++u) {
    if (qi[u] < l) {
      const float inv = 1.0f / lsum[u];
#pragma unroll
      for (int i = 0; i < D; ++i) op[(size_t)i * l + qi[u]] = o[u][i] * inv;
      // log2-domain log-sum-exp of the scaled scores (training saves it for the backward recompute)
      if (lse) lse[((size_t)n * heads + h) * l + qi[u]] = m[u] + log2f(lsum[u]);
    }
  }
}


// ---------------------------------------------------------------------------------------------------
// head_dim 8 on the matrix cores (the mid-block / Attn*Block2D case of the reference nets: 64 heads x 8).
// K = d = 8 is exactly one v_mfma_f32_32x32x8_f16 step, and the C/D layout of the 32x32 tile (lane = column,
// register r = row (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) is, for r = 4b .. 4b + 3, exactly the B-operand layout of
// the next 8-deep step.  So with S^T = K^T Q (rows = keys, columns = queries):
//   * a lane owns ONE query and 16 of the tile's 32 keys: the softmax is per lane, one exchange with lane ^ 32;
//   * P^T stays in registers and feeds O = V P as B operands (two 16-deep steps, V read in the matching key order)
//     -- no shuffles, no LDS round trip;
//   * V is the A operand with rows = the 8 head dims, a row of ONES (row 8 of the tile) accumulates the softmax
//     denominator of exactly the P that was multiplied, the other rows are padding.
// fp32-class accuracy as in conv_h2.hip: q, k, v and p are split x = hi + lo * 2^-11 (two fp16 parts), three MFMAs
// per product, the 2^11-scaled cross terms in a second accumulator (att_mfma8.h: operands, products, LDS images).
// Workgroup = 8 waves x 32 queries of one (image, head); its K and V (fp16 pairs) sit in LDS, KT keys at a time.
// ---------------------------------------------------------------------------------------------------
#ifndef DSG_ATM_MINW
#define DSG_ATM_MINW 4
#endif

// PREC 0: fp32-class accuracy (fp16 pairs, three MFMAs per product).  PREC 1 / 2 (the mixed-precision modes,
// BASELINE.json configs[4] "MFMA bf16 attn"): q, k, v and the probabilities are rounded once to bf16 / fp16, ONE MFMA per
// product, fp32 scores / running maximum / accumulators; the row of ones in V still accumulates the denominator of
// exactly the (rounded) probabilities that were multiplied, so each output row is a convex combination of V rows.
// BLK: q, k, v and the output are CHANNEL-BLOCKED, [N][3C/8][L][8] / [N][C/8][L][8] in the plan's element type (fp32, or
// the 16-bit type of PREC): head_dim 8 is exactly one channel block, so a token's q / k / v vector is one 32- / 16-byte
// piece -- the projection in front writes 16-byte pieces instead of scattering 4-byte words over 3C planes (its kernel
// ran at 0.8-1.2 TB/s), the K / V tiles load as whole vectors, and the out-projection behind reads blocked sources.
template <int PREC, bool BLK = false>
__global__ __launch_bounds__(64 * ATM_NW, DSG_ATM_MINW) void attention_mfma8_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                 float* __restrict__ lse, int c, int heads, int l,
                                                                 float qscale) {
  constexpr bool SPLIT = PREC == 0;
  constexpr bool E16 = BLK && PREC != 0;        // 16-bit elements
  constexpr int ESZ = E16 ? 2 : 4;
  typedef unsigned att_u2 __attribute__((ext_vector_type(2)));
  typedef unsigned att_u4 __attribute__((ext_vector_type(4)));
  // 8 consecutive elements of a blocked tensor as fp32
  auto load8 = [&](const char* ptr, float (&v)[8]) {
    if constexpr (E16) {
      const att_u4 w = *reinterpret_cast<const att_u4*>(ptr);
      v[0] = lo16<PREC>(w.x); v[1] = hi16<PREC>(w.x); v[2] = lo16<PREC>(w.y); v[3] = hi16<PREC>(w.y);
      v[4] = lo16<PREC>(w.z); v[5] = hi16<PREC>(w.z); v[6] = lo16<PREC>(w.w); v[7] = hi16<PREC>(w.w);
    } else {
      const float4 a = *reinterpret_cast<const float4*>(ptr), b = *reinterpret_cast<const float4*>(ptr + 16);
      v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
    }
  };
  __shared__ __attribute__((aligned(16))) _Float16 Kh[ATM_KT * 8], Kl[SPLIT ? ATM_KT * 8 : 8];          // [key][d]
  __shared__ __attribute__((aligned(16))) _Float16 Vh[9 * ATM_VSTR], Vl[SPLIT ? 9 * ATM_VSTR : 8];      // [d | ones][key]
  const att_image<SPLIT, false> K(Kh, Kl);
  const att_image<SPLIT, true> V(Vh, Vl);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const att_tile wg = att_tile_id(l, heads);   // (tile = 32 * ATM_NW queries)
  const int h = wg.h, n = wg.n;
  const float* qp = qkv + ((size_t)n * 3 * c + h * 8) * l;
  const float* kp = qp + (size_t)c * l;
  const float* vp = kp + (size_t)c * l;
  // blocked: channel block h of the q / k / v thirds of image n, [L][8] elements each
  const char* qb = reinterpret_cast<const char*>(qkv) + ((size_t)n * 3 * c + h * 8) * l * ESZ;
  const char* kb = qb + (size_t)c * l * ESZ;
  const char* vb = kb + (size_t)c * l * ESZ;
  const int q0 = (wg.tile * ATM_NW + wave) * 32;  // this wave's 32 queries (l % 32 == 0; a wave past the end idles)
  const bool active = q0 < l;
  const int qi = min(q0 + l31, l - 1);

  // B operand of S^T = K^T Q: lane (query l31, half) holds d = 4 half .. 4 half + 3, pre-scaled into the log2 domain
  att_h4<SPLIT> q;
  float qv8[8];
  if constexpr (BLK) load8(qb + (size_t)qi * 8 * ESZ, qv8);
#pragma unroll
  for (int i = 0; i < 4; ++i)
    q.set(i, att_split<PREC>((BLK ? (half ? qv8[4 + i] : qv8[i]) : qp[(size_t)(4 * half + i) * l + qi]) * qscale));
  att_acc<SPLIT> o = {};
  float m = -1e30f;
  const int vrow = min(l31, 8);  // A operand of O = V P: row = head dim (8 = the ones row, beyond: its copy, ignored)
  const att_h1<SPLIT> one = att_split<PREC>(1.0f), zero = att_split<PREC>(0.0f);

  for (int j0 = 0; j0 < l; j0 += ATM_KT) {
    const int kt = min(ATM_KT, l - j0);
    __syncthreads();
    if constexpr (BLK) {  // one key per thread: its k and v vectors are one piece each
      for (int j = tid; j < ATM_KT; j += 64 * ATM_NW) {
        float kv[8], vv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) kv[i] = vv[i] = 0.f;
        if (j < kt) {
          load8(kb + (size_t)(j0 + j) * 8 * ESZ, kv);
          load8(vb + (size_t)(j0 + j) * 8 * ESZ, vv);
        }
        att_h8<SPLIT> k8;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          k8.set(i, att_split<PREC>(kv[i]));
          V.store(j, i, att_split<PREC>(vv[i]));
        }
        K.store_row(j, k8);
      }
    } else {
      att_stage<PREC>(kp, 1.f, vp, 1.f, l, j0, kt, [&](int j, int i, att_h1<SPLIT> k, att_h1<SPLIT> v) {
        K.store(j, i, k);
        V.store(j, i, v);
      });
    }
    for (int j = tid; j < ATM_KT; j += 64 * ATM_NW) V.store(j, 8, j < kt ? one : zero);   // the ones row
    __syncthreads();
    if (!active) continue;
    // S^T tile = 32 keys x 32 queries; the NEXT tile's MFMAs are issued before this tile's softmax arithmetic
    // so that the matrix pipe works under it
    auto s_tile = [&](int t) { return att_prod8<PREC>(K.a_operand(t), q); };
    // one tile's softmax and O += V P from the scores in s
    auto pv_tile = [&](int t, const att_acc<SPLIT>& s) {
      float sv[16];
      float mx = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        sv[r] = s.value(r);
        mx = fmaxf(mx, sv[r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32, 64));  // the query's other 16 keys live in lane ^ 32
      const float mn = fmaxf(m, mx);
      const float sc = __builtin_amdgcn_exp2f(m - mn);  // (bare v_exp_f32: arguments <= 0, a flushed denormal is 0)
      m = mn;
#pragma unroll
      for (int r = 0; r < 5; ++r) {  // rows 0..3 (+4 half) = the head dims, row 8 (r = 4, half 0) = the denominator
        o.hi[r] *= sc;
        if constexpr (SPLIT) o.lo[r] *= sc;
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        // Registers 8 b .. 8 b + 7 are keys {0..3, 8..11} + 4 half of the tile's b-th 16 keys: as the B operand of a
        // 16-deep MFMA step they only need V (the A operand) read in the same key order.
        att_h8<SPLIT> p;
#pragma unroll
        for (int i = 0; i < 8; ++i) p.set(i, att_split<PREC>(__builtin_amdgcn_exp2f(sv[8 * b + i] - mn)));
        o = att_prod16<PREC>(V.frag16(vrow, t, b), p, o);
      }
    };
    // two score sets alternate (no register copies): while one tile's arithmetic runs, the other's MFMAs are in flight
    att_acc<SPLIT> sa = s_tile(0), sb;
    int t = 0;
    for (; t + 64 <= kt; t += 64) {  // (kt % 32 == 0)
      sb = s_tile(t + 32);
      pv_tile(t, sa);
      sa = s_tile(min(t + 64, kt - 32));  // (past the end: a tile that is not used)
      pv_tile(t + 32, sb);
    }
    if (t < kt) pv_tile(t, sa);  // odd tile count
  }
  if (!active) return;
  // row 8 of the tile (register 4 of the lower half-wave) is the denominator; the upper half-wave fetches it
  const float den_lo = o.value(4);  // (meaningful in the lower half-wave only)
  const float den_x = __shfl_xor(den_lo, 32, 64);
  const float den = half ? den_x : den_lo;
  const float inv = 1.0f / den;
  if (q0 + l31 < l) {
    float o4[4];  // this lane's four head dims of its query
#pragma unroll
    for (int r = 0; r < 4; ++r) o4[r] = o.value(r) * inv;
    if constexpr (BLK) {  // ... are one 16- / 8-byte piece of the token's channel block
      char* ob = reinterpret_cast<char*>(out) + ((((size_t)n * c + h * 8) * l + (size_t)(q0 + l31) * 8) + 4 * half) * ESZ;
      if constexpr (E16) *reinterpret_cast<att_u2*>(ob) = att_u2{pack2<PREC>(o4[0], o4[1]), pack2<PREC>(o4[2], o4[3])};
      else *reinterpret_cast<float4*>(ob) = make_float4(o4[0], o4[1], o4[2], o4[3]);
    } else {
      float* op = out + ((size_t)n * c + h * 8) * l;
#pragma unroll
      for (int r = 0; r < 4; ++r) op[(size_t)(r + 4 * half) * l + q0 + l31] = o4[r];
    }
    if (lse && half == 0) lse[((size_t)n * heads + h) * l + q0 + l31] = m + log2f(den);
  }
}

bool attention_blocked_ok(int c, int heads, int l) {
  return g_tune.att_mfma && g_tune.att_blocked && heads > 0 && c % heads == 0 && c / heads == 8 && l % 32 == 0;
}

// exact: keep off the fp16x2-split matrix-core kernel (q, k, v beyond fp16's range: the plan's range guard)
// dt: dsg_dtype of the products (DSG_F32 = the fp32-class split)
template <int D>
static int launch_attention(const float* qkv, float* out, float* lse, int n, int c, int heads, int l, hipStream_t st,
                            bool exact, int dt = DSG_F32) {
  // scores are kept in the log2 domain: q is pre-scaled by log2(e)/sqrt(D)
  const float qscale = 1.4426950408889634f / sqrtf((float)D);
  if (D == 8 && g_tune.att_mfma && !exact && l % 32 == 0) {
    const dim3 grid(cdiv(l, 32 * ATM_NW) * heads * n), block(64 * ATM_NW);
    if (dt == DSG_BF16) hipLaunchKernelGGL(attention_mfma8_kernel<1>, grid, block, 0, st, qkv, out, lse, c, heads, l, qscale);
    else if (dt == DSG_F16) hipLaunchKernelGGL(attention_mfma8_kernel<2>, grid, block, 0, st, qkv, out, lse, c, heads, l, qscale);
    else hipLaunchKernelGGL(attention_mfma8_kernel<0>, grid, block, 0, st, qkv, out, lse, c, heads, l, qscale);
    DSG_LAUNCH_CHECK();
    return DSG_OK;
  }
  const long work = (long)n * heads * l;
  int qpt = 4;
  if (work / (256 * 4) < 512) qpt = 2;
  if (work / (256 * 2) < 512) qpt = 1;
  if (D > 16) qpt = 1;
  dim3 grid(cdiv(l, 256 * qpt), heads, n);
  if constexpr (D <= 16) {  // wider heads keep one query per thread (register budget)
    if (qpt == 4) {
      hipLaunchKernelGGL((attention_kernel<D, 4>), grid, dim3(256), 0, st, qkv, out, lse, c, heads, l, qscale);
      DSG_LAUNCH_CHECK();
      return DSG_OK;
    }
    if (qpt == 2) {
      hipLaunchKernelGGL((attention_kernel<D, 2>), grid, dim3(256), 0, st, qkv, out, lse, c, heads, l, qscale);
      DSG_LAUNCH_CHECK();
      return DSG_OK;
    }
  }
  hipLaunchKernelGGL((attention_kernel<D, 1>), grid, dim3(256), 0, st, qkv, out, lse, c, heads, l, qscale);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

}  // namespace dsg

static int attention_fwd_impl(const float* qkv, float* out, float* lse, int32_t n, int32_t c, int32_t heads, int32_t l,
                              void* stream, bool exact = false, int dt = DSG_F32) {
  DSG_CHECK_ARG(qkv && out, "dsg_attention_fwd: NULL pointer");
  DSG_CHECK_ARG(n > 0 && c > 0 && heads > 0 && l > 0, "dsg_attention_fwd: bad dims");
  DSG_CHECK_ARG(c % heads == 0, "dsg_attention_fwd: channels (%d) not divisible by heads (%d)", c, heads);
  DSG_CHECK_ARG(heads <= 65535 && n <= 65535, "dsg_attention_fwd: grid too large");
  const int d = c / heads;
  hipStream_t st = static_cast<hipStream_t>(stream);
  switch (d) {
    case 8: return dsg::launch_attention<8>(qkv, out, lse, n, c, heads, l, st, exact, dt);
    case 16: return dsg::launch_attention<16>(qkv, out, lse, n, c, heads, l, st, exact);
    case 32: return dsg::launch_attention<32>(qkv, out, lse, n, c, heads, l, st, exact);
    case 64: return dsg::launch_attention<64>(qkv, out, lse, n, c, heads, l, st, exact);
    default:
      return dsg::fail(DSG_ERR_UNSUPPORTED_SHAPE, "dsg_attention_fwd: head_dim %d not in {8,16,32,64}", d);
  }
}

namespace dsg {
// the plan's range guard: q / k / v projections whose weights left the split's range run the fp32 VALU kernel
int attention_fwd_exact(const float* qkv, float* out, int n, int c, int heads, int l, hipStream_t st) {
  return attention_fwd_impl(qkv, out, nullptr, n, c, heads, l, st, true);
}
}  // namespace dsg

DSG_API int dsg_attention_fwd(const float* qkv, float* out, int32_t n, int32_t c, int32_t heads, int32_t l,
                              void* stream) {
  return attention_fwd_impl(qkv, out, nullptr, n, c, heads, l, stream);
}

DSG_API int dsg_attention_fwd_dt(const float* qkv, float* out, int32_t n, int32_t c, int32_t heads, int32_t l,
                                 int32_t dtype, void* stream) {
  DSG_CHECK_ARG(dtype >= DSG_F32 && dtype <= DSG_F16, "dsg_attention_fwd_dt: bad dtype %d", dtype);
  return attention_fwd_impl(qkv, out, nullptr, n, c, heads, l, stream, false, dtype);
}

// the same on channel-blocked tensors (see attention_mfma8_kernel<PREC, BLK>): head_dim 8, l % 32 == 0 only
DSG_API int dsg_attention_fwd_blocked(const void* qkv, void* out, int32_t n, int32_t c, int32_t heads, int32_t l,
                                      int32_t dtype, void* stream) {
  DSG_CHECK_ARG(qkv && out, "dsg_attention_fwd_blocked: NULL pointer");
  DSG_CHECK_ARG(dtype >= DSG_F32 && dtype <= DSG_F16, "dsg_attention_fwd_blocked: bad dtype %d", dtype);
  DSG_CHECK_ARG(n > 0 && c > 0 && heads > 0 && l > 0 && c % heads == 0, "dsg_attention_fwd_blocked: bad dims");
  DSG_CHECK_SHAPE(c / heads == 8 && l % 32 == 0,
                  "dsg_attention_fwd_blocked: head_dim %d / %d tokens (needs head_dim 8 = one channel block, tokens %% 32 == 0)",
                  c / heads, l);
  const float qscale = 1.4426950408889634f / sqrtf(8.0f);
  const dim3 grid(dsg::cdiv(l, 32 * dsg::ATM_NW) * heads * n), block(64 * dsg::ATM_NW);
  hipStream_t st = static_cast<hipStream_t>(stream);
  const float* q = static_cast<const float*>(qkv);
  float* o = static_cast<float*>(out);
  if (dtype == DSG_BF16) hipLaunchKernelGGL((dsg::attention_mfma8_kernel<1, true>), grid, block, 0, st, q, o, nullptr, c, heads, l, qscale);
  else if (dtype == DSG_F16) hipLaunchKernelGGL((dsg::attention_mfma8_kernel<2, true>), grid, block, 0, st, q, o, nullptr, c, heads, l, qscale);
  else hipLaunchKernelGGL((dsg::attention_mfma8_kernel<0, true>), grid, block, 0, st, q, o, nullptr, c, heads, l, qscale);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_attention_fwd_train(const float* qkv, float* out, float* lse, int32_t n, int32_t c, int32_t heads,
                                    int32_t l, void* stream) {
  DSG_CHECK_ARG(lse != nullptr, "dsg_attention_fwd_train: lse is NULL");
  return attention_fwd_impl(qkv, out, lse, n, c, heads, l, stream);
}

// the same in the arithmetic of the mixed-precision tape (DSG_BF16: the forward of dsg_attention_bwd_dt's matrix-core kernels --
// both round q * scale and k alike, so the backward recomputes exactly the probabilities the forward used)
DSG_API int dsg_attention_fwd_train_dt(const float* qkv, float* out, float* lse, int32_t n, int32_t c, int32_t heads,
                                       int32_t l, int32_t dtype, void* stream) {
  DSG_CHECK_ARG(lse != nullptr, "dsg_attention_fwd_train_dt: lse is NULL");
  DSG_CHECK_ARG(dtype >= DSG_F32 && dtype <= DSG_F16, "dsg_attention_fwd_train_dt: bad dtype %d", dtype);
  return attention_fwd_impl(qkv, out, lse, n, c, heads, l, stream, false, dtype);
}

// ---------------------------------------------------------------------------------------------------
// Backward of the attention core (flash-style recompute from the saved log-sum-exp):
//   P = exp2(s - lse), dP = dO . V, dS = P * (dP - D), D = rowsum(dO * O)
//   dQ = dS K * scale, dK = dS^T Q * scale, dV = P^T dO
// Kernel A: one thread per query row (keys/values streamed through LDS) -> dQ and D.
// Kernel B: one thread per key row (queries / dO / lse / D streamed through LDS) -> dK, dV.
// ---------------------------------------------------------------------------------------------------
namespace dsg {

typedef float att_f2 __attribute__((ext_vector_type(2)));

template <int D>
__global__ __launch_bounds__(256) void attention_bwd_dq_kernel(const float* __restrict__ qkv,
                                                               const float* __restrict__ o,
                                                               const float* __restrict__ dout,
                                                               const float* __restrict__ lse, float* __restrict__ dqkv,
                                                               float* __restrict__ dsum, int c, int heads, int l,
                                                               float qscale) {
  constexpr int KT = ATT_LDS_FLOATS / D;
  __shared__ __attribute__((aligned(16))) float KVl[2 * KT * D];
  float* Kl = KVl;
  float* Vl = KVl + KT * D;
  const int tid = threadIdx.x;
  const int h = blockIdx.y, n = blockIdx.z;
  const float* qp = qkv + ((size_t)n * 3 * c + h * D) * l;
  const float* kp = qp + (size_t)c * l;
  const float* vp = kp + (size_t)c * l;
  const size_t obase = ((size_t)n * c + h * D) * l;
  const int qi = blockIdx.x * 256 + tid;
  const int qc = min(qi, l - 1);
  float q[D], dO[D], dq[D];
  att_f2 dq2[D];  // (even keys, odd keys)
#pragma unroll
  for (int i = 0; i < D; ++i) dq2[i] = att_f2{0.f, 0.f};
  float dd = 0.f;
#pragma unroll
  for (int i = 0; i < D; ++i) {
    q[i] = qp[(size_t)i * l + qc] * qscale;
    dO[i] = dout[obase + (size_t)i * l + qc];
    dd = fmaf(dO[i], o[obase + (size_t)i * l + qc], dd);
    dq[i] = 0.f;
  }
  const float ls = lse[((size_t)n * heads + h) * l + qc];
  for (int j0 = 0; j0 < l; j0 += KT) {
    const int kt = min(KT, l - j0);
    __syncthreads();
    for (int e = tid; e < KT * D; e += 256) {
      const int i = e / KT, j = e - i * KT;
      float kv = 0.f, vv = 0.f;
      if (j < kt) {
        kv = kp[(size_t)i * l + j0 + j];
        vv = vp[(size_t)i * l + j0 + j];
      }
      // key PAIRS side by side: [pair][dim][2] -- the loop below works on two keys per packed fp32 instruction
      Kl[((j >> 1) * D + i) * 2 + (j & 1)] = kv;
      Vl[((j >> 1) * D + i) * 2 + (j & 1)] = vv;
    }
    __syncthreads();
    // (a padded key has K = V = 0: its probability is not zero, but everything it is multiplied into dq by is)
    // (the pair's K and V rows are fetched one iteration ahead into a second register set -- consumed as they are read,
    // the broadcast LDS reads' latency was most of an iteration; two sets taking turns, no copies)
    const int npair = (kt + 1) / 2;
    const att_f2* K2 = reinterpret_cast<const att_f2*>(Kl);
    const att_f2* V2 = reinterpret_cast<const att_f2*>(Vl);
    auto fetch = [&](int jp, att_f2 (&kr)[D], att_f2 (&vr)[D]) {
      const int jc = min(jp, npair - 1);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        kr[i] = K2[jc * D + i];
        vr[i] = V2[jc * D + i];
      }
    };
    auto pair = [&](const att_f2 (&kr)[D], const att_f2 (&vr)[D]) {
      att_f2 s = {0.f, 0.f}, dp = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < D; ++i) {
        s = __builtin_elementwise_fma(att_f2{q[i], q[i]}, kr[i], s);
        dp = __builtin_elementwise_fma(att_f2{dO[i], dO[i]}, vr[i], dp);
      }
      const att_f2 pr = {__builtin_amdgcn_exp2f(s.x - ls), __builtin_amdgcn_exp2f(s.y - ls)};  // (arguments <= ~0)
      const att_f2 ds = pr * (dp - att_f2{dd, dd});
#pragma unroll
      for (int i = 0; i < D; ++i) dq2[i] = __builtin_elementwise_fma(ds, kr[i], dq2[i]);
    };
    att_f2 ka[D], va[D], kb[D], vb[D];
    fetch(0, ka, va);
    int jp = 0;
    for (; jp + 1 < npair; jp += 2) {
      fetch(jp + 1, kb, vb);
      pair(ka, va);
      fetch(jp + 2, ka, va);
      pair(kb, vb);
    }
    if (jp < npair) pair(ka, va);
  }
#pragma unroll
  for (int i = 0; i < D; ++i) dq[i] = dq2[i].x + dq2[i].y;
  if (qi < l) {
    // qscale = log2(e)/sqrt(D); the softmax scale alone is 1/sqrt(D)
    const float sm = qscale * 0.6931471805599453f;
    float* dqp = dqkv + ((size_t)n * 3 * c + h * D) * l;
#pragma unroll
    for (int i = 0; i < D; ++i) dqp[(size_t)i * l + qi] = dq[i] * sm;
    dsum[((size_t)n * heads + h) * l + qi] = dd;
  }
}

template <int D>
__global__ __launch_bounds__(256) void attention_bwd_dkv_kernel(const float* __restrict__ qkv,
                                                                const float* __restrict__ dout,
                                                                const float* __restrict__ lse,
                                                                const float* __restrict__ dsum,
                                                                float* __restrict__ dqkv, int c, int heads, int l,
                                                                float qscale) {
  constexpr int QT = (ATT_LDS_FLOATS / (D + 1)) & ~1;  // queries per LDS tile (even: they sit in pairs): q[D], dO[D], lse, D-sum
  __shared__ __attribute__((aligned(16))) float Sm[2 * QT * (D + 1)];
  float* Ql = Sm;                  // [QT][D+1]: q (prescaled) then lse
  float* Gl = Sm + QT * (D + 1);   // [QT][D+1]: dO then dsum
  const int tid = threadIdx.x;
  const int h = blockIdx.y, n = blockIdx.z;
  const float* qp = qkv + ((size_t)n * 3 * c + h * D) * l;
  const float* kp = qp + (size_t)c * l;
  const float* vp = kp + (size_t)c * l;
  const size_t obase = ((size_t)n * c + h * D) * l;
  const size_t lbase = ((size_t)n * heads + h) * l;
  const int ki = blockIdx.x * 256 + tid;
  const int kc = min(ki, l - 1);
  float k[D], v[D], dk[D], dv[D];
  att_f2 dk2[D], dv2[D];  // (even queries, odd queries)
#pragma unroll
  for (int i = 0; i < D; ++i) dk2[i] = dv2[i] = att_f2{0.f, 0.f};
#pragma unroll
  for (int i = 0; i < D; ++i) {
    k[i] = kp[(size_t)i * l + kc];
    v[i] = vp[(size_t)i * l + kc];
    dk[i] = 0.f;
    dv[i] = 0.f;
  }
  for (int j0 = 0; j0 < l; j0 += QT) {
    const int qt = min(QT, l - j0);
    __syncthreads();
    for (int e = tid; e < QT * (D + 1); e += 256) {
      const int i = e / QT, j = e - i * QT;
      float a = 0.f, b = 0.f;
      if (j < qt) {
        if (i < D) {
          a = qp[(size_t)i * l + j0 + j] * qscale;
          b = dout[obase + (size_t)i * l + j0 + j];
        } else {
          a = lse[lbase + j0 + j];
          b = dsum[lbase + j0 + j];
        }
      }
      // query PAIRS side by side: [pair][dim + 1][2]
      Ql[((j >> 1) * (D + 1) + i) * 2 + (j & 1)] = a;
      Gl[((j >> 1) * (D + 1) + i) * 2 + (j & 1)] = b;
    }
    __syncthreads();
    // (a padded query has q = dO = lse = D-sum = 0: whatever its probability, it adds 0 to dk and dv)
    const int npair = (qt + 1) / 2;
    const att_f2* Q2 = reinterpret_cast<const att_f2*>(Ql);
    const att_f2* G2 = reinterpret_cast<const att_f2*>(Gl);
    auto fetch = [&](int jp, att_f2 (&qr)[D + 1], att_f2 (&gr)[D + 1]) {
      const int jc = min(jp, npair - 1);
#pragma unroll
      for (int i = 0; i <= D; ++i) {
        qr[i] = Q2[jc * (D + 1) + i];
        gr[i] = G2[jc * (D + 1) + i];
      }
    };
    auto pair = [&](const att_f2 (&qr)[D + 1], const att_f2 (&gr)[D + 1]) {
      att_f2 s = {0.f, 0.f}, dp = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < D; ++i) {
        s = __builtin_elementwise_fma(qr[i], att_f2{k[i], k[i]}, s);
        dp = __builtin_elementwise_fma(gr[i], att_f2{v[i], v[i]}, dp);
      }
      const att_f2 e = s - qr[D];
      const att_f2 pr = {__builtin_amdgcn_exp2f(e.x), __builtin_amdgcn_exp2f(e.y)};
      const att_f2 ds = pr * (dp - gr[D]);
#pragma unroll
      for (int i = 0; i < D; ++i) {
        dv2[i] = __builtin_elementwise_fma(pr, gr[i], dv2[i]);
        dk2[i] = __builtin_elementwise_fma(ds, qr[i], dk2[i]);  // qr is prescaled by log2(e)/sqrt(D): undone below
      }
    };
    att_f2 qa[D + 1], ga[D + 1], qb[D + 1], gb[D + 1];
    fetch(0, qa, ga);
    int jp = 0;
    for (; jp + 1 < npair; jp += 2) {
      fetch(jp + 1, qb, gb);
      pair(qa, ga);
      fetch(jp + 2, qa, ga);
      pair(qb, gb);
    }
    if (jp < npair) pair(qa, ga);
  }
#pragma unroll
  for (int i = 0; i < D; ++i) {
    dk[i] = dk2[i].x + dk2[i].y;
    dv[i] = dv2[i].x + dv2[i].y;
  }
  if (ki < l) {
    float* dkp = dqkv + ((size_t)n * 3 * c + c + h * D) * l;
    float* dvp = dkp + (size_t)c * l;
#pragma unroll
    for (int i = 0; i < D; ++i) {
      dkp[(size_t)i * l + ki] = dk[i] * 0.6931471805599453f;
      dvp[(size_t)i * l + ki] = dv[i];
    }
  }
}

// ---------------------------------------------------------------------------------------------------
// The same backward on the matrix cores for head_dim 8 in the mixed-precision tapes: q, k, v, dO, P and dS are rounded
// once to 16 bits, one MFMA per product (PREC 1: bf16.  PREC 2, the fp16 tape: dS = P (dP - D) is a probability times a
// gradient, 1e-3 x 1e-6 without a loss scale -- below fp16's normal range, flushed bits that the test of a whole training step
// caught.  The gradients are linear in dO, so dO is multiplied by a power of two that brings its largest entry to [1, 2) before
// it is rounded and the results are divided by it: per query in kernel A, per (image, head) in kernel B, whose sums run over the
// queries), fp32 scores / accumulators -- torch.autocast's split for the attention core (the fp32 tape
// keeps the exact VALU kernels above: with fp16-pair operands the split arithmetic would cost what the packed-fp32 loops do).
// Layouts are the forward kernel's (attention_mfma8_kernel): a 32 x 32 tile of S^T = K^T Q leaves a lane with ONE column and 16
// rows, and registers 8b .. 8b + 7 are the B operand of a 16-deep step over those rows.
//   kernel A (dQ): columns = this wave's 32 queries (q, dO, lse, D = rowsum(dO * O) live in registers), rows = keys from LDS:
//                  S^T = K^T Q, dP^T = V^T dO, dS = P (dP - D), dQ^T += K^T(as [d][key]) dS
//   kernel B (dK, dV): columns = this wave's 32 keys, rows = queries from LDS (with their lse and D):
//                  S = Q^T K, dP = dO^T V, dV^T += dO(as [d][query]) P, dK^T += Q(as [d][query]) dS
// ---------------------------------------------------------------------------------------------------
// PREC 0 (round 6; the fp32 tape's attention backward, training_pipeline.py:86 through the mid block's Attention): every product
// as the fp16x2 split -- a.b ~ a1.b1 + 2^-11 (a1.b2 + a2.b1), three MFMAs, the cross terms on accumulators of their own -- with
// dO brought to [1, 2) by a power of two first (the pieces are fp16: unscaled gradients of 1e-6 would land in its subnormals).
// fp32-class accuracy (tests/test_gpu_train_ops.py: 2e-5 against torch autograd, the VALU kernels' own tolerance) on the
// matrix cores: the fp32 tape's two VALU kernels were 6.5 ms of the configs[2] step.
template <int PREC>
__global__ __launch_bounds__(64 * ATM_NW, 2) void attention_bwd_dq_mfma8_kernel(const float* __restrict__ qkv, const float* __restrict__ o,
                                                                               const float* __restrict__ dout, const float* __restrict__ lse,
                                                                               float* __restrict__ dqkv, float* __restrict__ dsum, int c,
                                                                               int heads, int l, float qscale) {
  constexpr bool SPLIT = PREC == 0;
  constexpr bool SCALE = PREC != 1;  // fp16 pieces: dO is brought to [1, 2) by a power of two before it is rounded (see above)
  __shared__ __attribute__((aligned(16))) _Float16 Kh[ATM_KT * 8], Vh[ATM_KT * 8];   // [key][d]: A operands of S^T and dP^T
  __shared__ __attribute__((aligned(16))) _Float16 Kdh[8 * ATM_VSTR];                 // [d][key]: A operand of dQ^T += K dS
  __shared__ __attribute__((aligned(16))) _Float16 Kl[SPLIT ? ATM_KT * 8 : 8], Vl[SPLIT ? ATM_KT * 8 : 8], Kdl[SPLIT ? 8 * ATM_VSTR : 8];
  const att_image<SPLIT, false> K(Kh, Kl), V(Vh, Vl);
  const att_image<SPLIT, true> Kd(Kdh, Kdl);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const att_tile wg = att_tile_id(l, heads);   // (tile = 32 * ATM_NW queries)
  const int h = wg.h, n = wg.n;
  const float* qp = qkv + ((size_t)n * 3 * c + h * 8) * l;
  const float* kp = qp + (size_t)c * l;
  const float* vp = kp + (size_t)c * l;
  const size_t obase = ((size_t)n * c + h * 8) * l;
  const int q0 = (wg.tile * ATM_NW + wave) * 32;
  const bool active = q0 < l;
  const int qi = min(q0 + l31, l - 1);
  att_h4<SPLIT> q, d;
  float dpart = 0.f;
  float dov4[4], amax = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const size_t at = (size_t)(4 * half + i) * l + qi;
    dov4[i] = dout[obase + at];
    q.set(i, att_split<PREC>(qp[at] * qscale));
    dpart = fmaf(dov4[i], o[obase + at], dpart);
    amax = fmaxf(amax, fabsf(dov4[i]));
  }
  // this query's power-of-two scale (lanes l31 and l31 + 32 hold its two halves): dQ_i is linear in dO_i, undone at the end
  float qs = 1.f, qs_inv = 1.f;
  if constexpr (SCALE) att_pow2_scale(fmaxf(amax, __shfl_xor(amax, 32, 64)), &qs, &qs_inv);
#pragma unroll
  for (int i = 0; i < 4; ++i) d.set(i, att_split<PREC>(dov4[i] * qs));
  const float dd_true = dpart + __shfl_xor(dpart, 32, 64);   // D = rowsum(dO * O) of this lane's query
  const float dd = dd_true * qs;
  const float ls = lse[((size_t)n * heads + h) * l + qi];
  att_acc<SPLIT> dq = {};
  const int vrow = min(l31, 7);
  for (int j0 = 0; j0 < l; j0 += ATM_KT) {
    const int kt = min(ATM_KT, l - j0);
    __syncthreads();
    att_stage<PREC>(kp, 1.f, vp, 1.f, l, j0, kt, [&](int j, int i, att_h1<SPLIT> k, att_h1<SPLIT> v) {
      K.store(j, i, k);
      Kd.store(j, i, k);
      V.store(j, i, v);
    });
    __syncthreads();
    if (!active) continue;
    for (int t = 0; t < kt; t += 32) {
      const att_acc<SPLIT> sc = att_prod8<PREC>(K.a_operand(t), q);   // S^T: rows = keys, this lane's column = its query
      const att_acc<SPLIT> dp = att_prod8<PREC>(V.a_operand(t), d);   // dP^T
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        att_h8<SPLIT> ds;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float pv = __builtin_amdgcn_exp2f(sc.value(8 * b + i) - ls);
          ds.set(i, att_split<PREC>(pv * (dp.value(8 * b + i) - dd)));
        }
        dq = att_prod16<PREC>(Kd.frag16(vrow, t, b), ds, dq);
      }
    }
  }
  if (!active || q0 + l31 >= l) return;
  const float sm = qscale * 0.6931471805599453f * qs_inv;  // qscale = log2(e)/sqrt(D); the softmax scale alone is 1/sqrt(D)
  float* dqp = dqkv + ((size_t)n * 3 * c + h * 8) * l;
#pragma unroll
  for (int r = 0; r < 4; ++r) dqp[(size_t)(r + 4 * half) * l + q0 + l31] = dq.value(r) * sm;
  if (half == 0) dsum[((size_t)n * heads + h) * l + q0 + l31] = dd_true;
}

template <int PREC>
__global__ __launch_bounds__(64 * ATM_NW, PREC == 0 ? 1 : 2) void attention_bwd_dkv_mfma8_kernel(const float* __restrict__ qkv, const float* __restrict__ dout,
                                                                                const float* __restrict__ lse, const float* __restrict__ dsum,
                                                                                float* __restrict__ dqkv, int c, int heads, int l,
                                                                                float qscale) {
  constexpr bool SPLIT = PREC == 0;  // fp32-class: every product as the fp16x2 split (see the dq kernel)
  constexpr bool SCALE = PREC != 1;  // fp16 pieces: dO is brought to [1, 2) by a power of two before it is rounded (see above)
  __shared__ __attribute__((aligned(16))) _Float16 Qh[ATM_KT * 8], Gh[ATM_KT * 8];            // [query][d]: A operands of S and dP
  __shared__ __attribute__((aligned(16))) _Float16 Qdh[8 * ATM_VSTR], Gdh[8 * ATM_VSTR];      // [d][query]: A operands of dK^T, dV^T
  __shared__ __attribute__((aligned(16))) _Float16 Ql[SPLIT ? ATM_KT * 8 : 8], Gl[SPLIT ? ATM_KT * 8 : 8];
  __shared__ __attribute__((aligned(16))) _Float16 Qdl[SPLIT ? 8 * ATM_VSTR : 8], Gdl[SPLIT ? 8 * ATM_VSTR : 8];
  __shared__ __attribute__((aligned(16))) float Ls[ATM_KT], Ds[ATM_KT];                        // lse and D of the tile's queries
  const att_image<SPLIT, false> Q(Qh, Ql), G(Gh, Gl);
  const att_image<SPLIT, true> Qd(Qdh, Qdl), Gd(Gdh, Gdl);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, half = lane >> 5, l31 = lane & 31;
  const att_tile wg = att_tile_id(l, heads);   // (tile = 32 * ATM_NW keys)
  const int h = wg.h, n = wg.n;
  const float* qp = qkv + ((size_t)n * 3 * c + h * 8) * l;
  const float* kp = qp + (size_t)c * l;
  const float* vp = kp + (size_t)c * l;
  const size_t obase = ((size_t)n * c + h * 8) * l;
  const size_t lbase = ((size_t)n * heads + h) * l;
  const int k0 = (wg.tile * ATM_NW + wave) * 32;
  const bool active = k0 < l;
  const int ki = min(k0 + l31, l - 1);
  att_h4<SPLIT> k, v;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    k.set(i, att_split<PREC>(kp[(size_t)(4 * half + i) * l + ki]));
    v.set(i, att_split<PREC>(vp[(size_t)(4 * half + i) * l + ki]));
  }
  // dK_j and dV_j sum over the queries: ONE scale for the head's whole dO (its 8 l values are contiguous; every workgroup of
  // the head finds the same maximum -- no atomics, no extra buffer); rows far below the maximum lose bits that do not show in the sum
  float gs = 1.f, gs_inv = 1.f;
  if constexpr (SCALE) {
    __shared__ float wmax[ATM_NW];
    float m = 0.f;
    for (int e = tid; e < 8 * l; e += 64 * ATM_NW) m = fmaxf(m, fabsf(dout[obase + e]));
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) m = fmaxf(m, __shfl_xor(m, sft, 64));
    if (lane == 0) wmax[wave] = m;
    __syncthreads();
    m = wmax[0];
#pragma unroll
    for (int w = 1; w < ATM_NW; ++w) m = fmaxf(m, wmax[w]);
    att_pow2_scale(m, &gs, &gs_inv);
  }
  att_acc<SPLIT> dk = {}, dv = {};
  const int vrow = min(l31, 7);
  for (int j0 = 0; j0 < l; j0 += ATM_KT) {
    const int qt = min(ATM_KT, l - j0);
    __syncthreads();
    att_stage<PREC>(qp, qscale, dout + obase, gs, l, j0, qt, [&](int j, int i, att_h1<SPLIT> q, att_h1<SPLIT> g) {
      Q.store(j, i, q);
      Qd.store(j, i, q);
      G.store(j, i, g);
      Gd.store(j, i, g);
    });
    for (int j = tid; j < ATM_KT; j += 64 * ATM_NW) {
      Ls[j] = j < qt ? lse[lbase + j0 + j] : 0.f;
      Ds[j] = j < qt ? dsum[lbase + j0 + j] * gs : 0.f;
    }
    __syncthreads();
    if (!active) continue;
    for (int t = 0; t < qt; t += 32) {
      const att_acc<SPLIT> sc = att_prod8<PREC>(Q.a_operand(t), k);   // S: rows = queries, this lane's column = its key
      const att_acc<SPLIT> dp = att_prod8<PREC>(G.a_operand(t), v);   // dP
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        // registers 8b .. 8b + 7 = queries t + 16 b + 4 half + {0..3, 8..11}
        const float4 l0 = *reinterpret_cast<const float4*>(&Ls[t + 16 * b + 4 * half]);
        const float4 l1 = *reinterpret_cast<const float4*>(&Ls[t + 16 * b + 4 * half + 8]);
        const float4 d0 = *reinterpret_cast<const float4*>(&Ds[t + 16 * b + 4 * half]);
        const float4 d1 = *reinterpret_cast<const float4*>(&Ds[t + 16 * b + 4 * half + 8]);
        const float lsr[8] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
        const float ddr[8] = {d0.x, d0.y, d0.z, d0.w, d1.x, d1.y, d1.z, d1.w};
        att_h8<SPLIT> p, ds;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float pv = __builtin_amdgcn_exp2f(sc.value(8 * b + i) - lsr[i]);
          p.set(i, att_split<PREC>(pv));
          ds.set(i, att_split<PREC>(pv * (dp.value(8 * b + i) - ddr[i])));
        }
        dv = att_prod16<PREC>(Gd.frag16(vrow, t, b), p, dv);
        dk = att_prod16<PREC>(Qd.frag16(vrow, t, b), ds, dk);
      }
    }
  }
  if (!active || k0 + l31 >= l) return;
  float* dkp = dqkv + ((size_t)n * 3 * c + c + h * 8) * l;
  float* dvp = dkp + (size_t)c * l;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dkp[(size_t)(r + 4 * half) * l + k0 + l31] = dk.value(r) * (0.6931471805599453f * gs_inv);  // (q came pre-scaled by log2(e)/sqrt(D))
    dvp[(size_t)(r + 4 * half) * l + k0 + l31] = dv.value(r) * gs_inv;
  }
}

template <int PREC>
static int launch_attention_bwd_mfma8(const float* qkv, const float* o, const float* dout, const float* lse, float* dqkv,
                                      float* dsum, int n, int c, int heads, int l, hipStream_t st) {
  const float qscale = 1.4426950408889634f / sqrtf(8.0f);
  const dim3 grid(cdiv(l, 32 * ATM_NW) * heads * n), block(64 * ATM_NW);
  hipLaunchKernelGGL(attention_bwd_dq_mfma8_kernel<PREC>, grid, block, 0, st, qkv, o, dout, lse, dqkv, dsum, c, heads, l, qscale);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(attention_bwd_dkv_mfma8_kernel<PREC>, grid, block, 0, st, qkv, dout, lse, dsum, dqkv, c, heads, l, qscale);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

template <int D>
static int launch_attention_bwd(const float* qkv, const float* o, const float* dout, const float* lse, float* dqkv,
                                float* dsum, int n, int c, int heads, int l, hipStream_t st) {
  const float qscale = 1.4426950408889634f / sqrtf((float)D);
  dim3 grid(cdiv(l, 256), heads, n);
  hipLaunchKernelGGL((attention_bwd_dq_kernel<D>), grid, dim3(256), 0, st, qkv, o, dout, lse, dqkv, dsum, c, heads, l,
                     qscale);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL((attention_bwd_dkv_kernel<D>), grid, dim3(256), 0, st, qkv, dout, lse, dsum, dqkv, c, heads, l,
                     qscale);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

}  // namespace dsg

// dtype: DSG_F32 = the exact kernels; DSG_BF16 / DSG_F16 = the matrix-core kernels (head_dim 8, l % 32 == 0; anything else: the
// exact ones).  DSG_F16: dO enters the fp16 products scaled by a power of two (kernel comments), whatever the loss scale is.
DSG_API int dsg_attention_bwd_dt(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                 float* dsum_ws, int32_t n, int32_t c, int32_t heads, int32_t l, int32_t dtype, void* stream) {
  DSG_CHECK_ARG(qkv && out && dout && lse && dqkv && dsum_ws, "dsg_attention_bwd_dt: NULL pointer");
  DSG_CHECK_ARG(n > 0 && c > 0 && heads > 0 && l > 0 && c % heads == 0, "dsg_attention_bwd_dt: bad dims");
  DSG_CHECK_ARG(dtype >= DSG_F32 && dtype <= DSG_F16, "dsg_attention_bwd_dt: bad dtype %d", dtype);
  if (dtype != DSG_F32 && c / heads == 8 && l % 32 == 0 && dsg::g_tune.att_mfma)
    return dtype == DSG_BF16
               ? dsg::launch_attention_bwd_mfma8<1>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, static_cast<hipStream_t>(stream))
               : dsg::launch_attention_bwd_mfma8<2>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, static_cast<hipStream_t>(stream));
  return dsg_attention_bwd(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, stream);
}

DSG_API int dsg_attention_bwd(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                              float* dsum_ws, int32_t n, int32_t c, int32_t heads, int32_t l, void* stream) {
  DSG_CHECK_ARG(qkv && out && dout && lse && dqkv && dsum_ws, "dsg_attention_bwd: NULL pointer");
  DSG_CHECK_ARG(n > 0 && c > 0 && heads > 0 && l > 0 && c % heads == 0, "dsg_attention_bwd: bad dims");
  DSG_CHECK_ARG(heads <= 65535 && n <= 65535, "dsg_attention_bwd: grid too large");
  hipStream_t st = static_cast<hipStream_t>(stream);
  // head_dim 8 (every attention block of the reference's networks): the matrix-core kernels in their fp32-class form (PREC 0);
  // tuning key 14 = 0 keeps the VALU kernels for A/B
  if (c / heads == 8 && l % 32 == 0 && dsg::g_tune.att_mfma && dsg::g_tune.att_bwd_split)
    return dsg::launch_attention_bwd_mfma8<0>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, st);
  switch (c / heads) {
    case 8: return dsg::launch_attention_bwd<8>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, st);
    case 16: return dsg::launch_attention_bwd<16>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, st);
    case 32: return dsg::launch_attention_bwd<32>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, st);
    case 64: return dsg::launch_attention_bwd<64>(qkv, out, dout, lse, dqkv, dsum_ws, n, c, heads, l, st);
    default:
      return dsg::fail(DSG_ERR_UNSUPPORTED_SHAPE, "dsg_attention_bwd: head_dim %d not in {8,16,32,64}", c / heads);
  }
}
