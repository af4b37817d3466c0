// Operand, product and LDS-image layer of the head_dim 8 matrix-core attention kernels (attention.hip: the forward and the
// backward pair).  All three work on 32 x 32 tiles whose 8-deep products take a [row][8] LDS image as the A operand and
// whose 16-deep products take a [8][row] image; in the fp32-class mode (PREC 0, SPLIT) every operand is an fp16 pair
// x = hi + lo * 2^-11 and every product three MFMAs.  The scheme is stated here once: the kernels name operands, not parts.
#pragma once
#include "dsg_h16.h"

namespace dsg {

typedef _Float16 att_half4 __attribute__((ext_vector_type(4)));
typedef _Float16 att_half8 __attribute__((ext_vector_type(8)));
typedef short att_short4 __attribute__((ext_vector_type(4)));
constexpr int ATM_KT = 512;                  // rows (keys / queries) per LDS tile (the forward: 35 KB of LDS, four workgroups per CU)
constexpr int ATM_VSTR = ATM_KT + 4;         // row stride of a [d][row] image in halfs (+8 bytes: rows fall into different banks)
constexpr int ATM_NW = 8;                    // waves per workgroup: 256 columns share one conversion of the tile

// fp32 -> the 16-bit operand type of PREC, carried in a _Float16-typed container (bits only)
template <int PREC>
__device__ __forceinline__ _Float16 att_cvt(float v) {
  if constexpr (PREC == 1) return __builtin_bit_cast(_Float16, (__bf16)v);
  else return (_Float16)v;
}
// one 8-deep step on the matrix cores
template <int PREC>
__device__ __forceinline__ f32x16 att_mma8(att_half4 a, att_half4 b, f32x16 c) {
  if constexpr (PREC == 1)
    return __builtin_amdgcn_mfma_f32_32x32x8bf16_1k(__builtin_bit_cast(att_short4, a), __builtin_bit_cast(att_short4, b), c, 0, 0, 0);
  else
    return __builtin_amdgcn_mfma_f32_32x32x8f16(a, b, c, 0, 0, 0);
}

// ---- operand pairs: `hi`, and with SPLIT a `lo` part (without it there is no such member, so it costs no register)
template <class V, bool SPLIT> struct att_parts { V hi, lo; };
template <class V> struct att_parts<V, false> { V hi; };
template <class V, bool SPLIT>
struct att_pair : att_parts<V, SPLIT> {
  // element i of a vector operand
  __device__ __forceinline__ void set(int i, att_pair<_Float16, SPLIT> s) {
    this->hi[i] = s.hi;
    if constexpr (SPLIT) this->lo[i] = s.lo;
  }
  // register r of an accumulator pair: the 2^11-scaled cross terms join here
  __device__ __forceinline__ float value(int r) const {
    if constexpr (SPLIT) return this->hi[r] + this->lo[r] * (1.0f / 2048.0f);
    else return this->hi[r];
  }
};
template <bool SPLIT> using att_h1 = att_pair<_Float16, SPLIT>;
template <bool SPLIT> using att_h4 = att_pair<att_half4, SPLIT>;   // A / B operand of an 8-deep step
template <bool SPLIT> using att_h8 = att_pair<att_half8, SPLIT>;   // ... of a 16-deep step
template <bool SPLIT> using att_acc = att_pair<f32x16, SPLIT>;

// PREC 0: (value, (value - hi) * 2^11) as an fp16 pair, x == hi + lo * 2^-11 to 2^-22 relative.  PREC 1 / 2: rounded once.
template <int PREC>
__device__ __forceinline__ att_h1<PREC == 0> att_split(float v) {
  if constexpr (PREC == 0) {
    const _Float16 h = (_Float16)v;
    return {{h, (_Float16)((v - (float)h) * 2048.0f)}};
  } else {
    return {{att_cvt<PREC>(v)}};
  }
}

// ---- products: hi.hi, then (SPLIT) hi.lo and lo.hi into the lo accumulator -- the only place that states this order
template <int PREC>
__device__ __forceinline__ att_acc<PREC == 0> att_prod8(att_h4<PREC == 0> a, att_h4<PREC == 0> b) {
  const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // (C = the inline constant 0)
  att_acc<PREC == 0> c;
  c.hi = att_mma8<PREC>(a.hi, b.hi, zero);
  if constexpr (PREC == 0) {
    c.lo = att_mma8<PREC>(a.hi, b.lo, zero);
    c.lo = att_mma8<PREC>(a.lo, b.hi, c.lo);
  }
  return c;
}
template <int PREC>
__device__ __forceinline__ att_acc<PREC == 0> att_prod16(att_h8<PREC == 0> a, att_h8<PREC == 0> b, att_acc<PREC == 0> c) {
  c.hi = mma16<PREC>(a.hi, b.hi, c.hi);
  if constexpr (PREC == 0) {
    c.lo = mma16<PREC>(a.hi, b.lo, c.lo);
    c.lo = mma16<PREC>(a.lo, b.hi, c.lo);
  }
  return c;
}

// ---- LDS images of a tile: element (row, d), d = 0..7 (the forward's V has a ninth d, its row of ones)
constexpr __host__ __device__ int att_image_at(bool dims, int row, int d) { return dims ? d * ATM_VSTR + row : row * 8 + d; }
// [row][8] image, A operand of an 8-deep step over rows t .. t + 31: lane (l31, half) holds d = 4 half .. 4 half + 3 of row t + l31
constexpr __host__ __device__ int att_a_operand_at(int t, int l31, int half) { return att_image_at(false, t + l31, 4 * half); }
// [d][row] image, A operand of the b-th 16-deep step over rows t .. t + 31: a C/D tile's registers 8 b .. 8 b + 7 are rows
// {0..3, 8..11} + 4 half of the tile's b-th 16, so the matching A operand is the four halfs here and the four at + 8
constexpr __host__ __device__ int att_frag16_at(int vrow, int t, int b, int half) { return att_image_at(true, t, vrow) + 16 * b + 4 * half; }
// staging: element e of the 8 * ATM_KT of a tile is (d, row) -- consecutive threads take consecutive rows of one [8][L] plane
constexpr __host__ __device__ int att_stage_d(int e) { return e / ATM_KT; }
constexpr __host__ __device__ int att_stage_row(int e) { return e - att_stage_d(e) * ATM_KT; }

// a view over caller-declared __shared__ arrays (hi, and lo with SPLIT); DIMS: [d][ATM_VSTR], else [row][8]
template <bool SPLIT, bool DIMS>
struct att_image {
  att_pair<_Float16*, SPLIT> p;
  int l31, half;   // this lane's column of the 32 x 32 tile and its half of the wave
  __device__ __forceinline__ att_image(_Float16* hi, _Float16* lo) : l31(threadIdx.x & 31), half((threadIdx.x & 63) >> 5) {
    p.hi = hi;
    if constexpr (SPLIT) p.lo = lo;
  }
  template <class V>
  __device__ __forceinline__ void put(int at, att_pair<V, SPLIT> v) const {
    *reinterpret_cast<V*>(&p.hi[at]) = v.hi;
    if constexpr (SPLIT) *reinterpret_cast<V*>(&p.lo[at]) = v.lo;
  }
  // (`plus` is added to the ADDRESS, not to the index: a constant the LDS instruction takes as its offset)
  template <class V>
  __device__ __forceinline__ att_pair<V, SPLIT> get(int at, int plus = 0) const {
    att_pair<V, SPLIT> v;
    v.hi = *reinterpret_cast<const V*>(&p.hi[at] + plus);
    if constexpr (SPLIT) v.lo = *reinterpret_cast<const V*>(&p.lo[at] + plus);
    return v;
  }
  __device__ __forceinline__ void store(int row, int d, att_h1<SPLIT> v) const { put(att_image_at(DIMS, row, d), v); }
  __device__ __forceinline__ void store_row(int row, att_h8<SPLIT> v) const {
    static_assert(!DIMS, "a row is contiguous in the [row][8] image only");
    put(att_image_at(false, row, 0), v);
  }
  __device__ __forceinline__ att_h4<SPLIT> a_operand(int t) const {
    static_assert(!DIMS, "8-deep A operands come from the [row][8] image");
    return get<att_half4>(att_a_operand_at(t, l31, half));
  }
  __device__ __forceinline__ att_h8<SPLIT> frag16(int vrow, int t, int b) const {
    static_assert(DIMS, "16-deep A operands come from the [d][row] image");
    const int at = att_frag16_at(vrow, t, b, half);
    const att_h4<SPLIT> x = get<att_half4>(at), y = get<att_half4>(at, 8);
    att_h8<SPLIT> v;
    v.hi = __builtin_shufflevector(x.hi, y.hi, 0, 1, 2, 3, 4, 5, 6, 7);
    if constexpr (SPLIT) v.lo = __builtin_shufflevector(x.lo, y.lo, 0, 1, 2, 3, 4, 5, 6, 7);
    return v;
  }
};

// Coalesced fill of one tile from two [8][L] fp32 planes: rows j0 .. j0 + kt - 1 of plane a times sa and of plane b times sb,
// zeros in the tile's rows past kt, split / rounded for PREC and handed to put(row, d, a, b), which stores them into its images
template <int PREC, class Put>
__device__ __forceinline__ void att_stage(const float* pa, float sa, const float* pb, float sb, int l, int j0, int kt, Put put) {
  for (int e = threadIdx.x; e < 8 * ATM_KT; e += 64 * ATM_NW) {
    const int i = att_stage_d(e), j = att_stage_row(e);
    float a = 0.f, b = 0.f;
    if (j < kt) {
      a = pa[(size_t)i * l + j0 + j] * sa;
      b = pb[(size_t)i * l + j0 + j] * sb;
    }
    put(j, i, att_split<PREC>(a), att_split<PREC>(b));
  }
}

// Workgroup id -> (tile of 32 * ATM_NW columns, head, image).  Consecutive ids go to the 8 XCDs in turn, each with its own L2:
// XCD k takes a CONTIGUOUS eighth of the (image, head, tile) list, so the tiles of one head -- which all stream the same
// K and V (q and dO) -- run behind one L2 at about the same time, and those come from HBM once instead of once per XCD
// (the tile-major order spread a head's 8 tiles over the 8 XCDs: 4.1x the algorithmic traffic, profiles/r01*).
struct att_tile { int tile, h, n; };
__device__ __forceinline__ att_tile att_tile_id(int l, int heads) {
  const int tiles = (l + 32 * ATM_NW - 1) / (32 * ATM_NW);
  int bid = blockIdx.x;
  if ((gridDim.x & 7) == 0) bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  const int hn = bid / tiles;
  return {bid % tiles, hn % heads, hn / heads};
}

// the power of two that brings amax to [1, 2), and its inverse (1 for amax = 0 / inf / NaN): fp16 pieces of dO stay normal
__device__ __forceinline__ void att_pow2_scale(float amax, float* s, float* inv) {
  *s = *inv = 1.f;
  if (amax > 0.f && amax < 3.0e38f) {
    int ex;
    (void)frexpf(amax, &ex);
    *s = ldexpf(1.0f, 1 - ex);
    *inv = ldexpf(1.0f, ex - 1);
  }
}

}  // namespace dsg
