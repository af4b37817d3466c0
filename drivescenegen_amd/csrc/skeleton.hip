// Skeleton stage of the vectoriser (continued): what the reference does with get_gray_image's lane mask
// next -- extract_network (DriveSceneGen/vectorization/graph/extract_network.py:270-277) thins it
// (`morphology.skeletonize`, :272) and classifies the skeleton's pixels in a per-pixel Python loop
// (`zhang_suen_node_detection`, :34-93, called at :240).  Two kernels, both one workgroup per image:
//
//  thin_lut_kernel     Two-sub-iteration parallel thinning driven by a 256-entry table (Zhang & Suen, CACM 27(3), 1984
//                      with the default table of imageops.zhang_suen_lut).  The image lives bit-packed in LDS for the whole
//                      call: rows of 32-bit words inside a one-word / one-row zero border, so a word's eight neighbour words
//                      are read without an edge test.  A 512 x 512 image is 514 x 18 words = 36.1 KiB (+ 9 KiB of bytes,
//                      below).  Thinning is IN PLACE: a sub-iteration computes every thread's new words into registers
//                      from the image as the previous sub-iteration left it, a barrier ends the reads, the changed words
//                      are stored, a barrier ends the stores.  Whether an iteration deleted anything is one LDS word that
//                      every thread reads after a barrier: the loop exit is uniform over the workgroup by construction,
//                      and bounded by max_iters.  An all-zero word costs one LDS read; a word whose 3 x 3 words have been
//                      still for two sub-iterations costs two (one "last change" byte per word): only the parts still
//                      eroding are looked at bit by bit.  Barrier- and LDS-latency-bound; one workgroup per image, so a
//                      small batch leaves most of the chip idle.
//  skel_nodes_kernel   A(p) = off->on steps round the 8-neighbourhood; a node is an on pixel with A = 1 or A >= 3.  Each
//                      wave owns a contiguous stretch of the row-major pixel order, counts its nodes (ballot + popcount)
//                      and keeps their positions in LDS, the wave totals are summed in order, and the coordinates are written
//                      at base + rank (a wave with more nodes than it keeps walks its stretch again): the list order is the
//                      array's row-major order, no atomics.
#include "dsg_common.h"

namespace dsg {

constexpr int THIN_THREADS = 1024;       // 16 waves: four per SIMD
constexpr int THIN_MAX_WORDS = 13;       // image words per thread (registers of the in-place update): instantiated for 4, 8, 13
constexpr size_t THIN_LDS_MAX = 65536;   // what a kernel may declare without raising its limit
constexpr int NODE_THREADS = 1024;

__host__ __device__ static inline size_t thin_lds_bytes(int h, int w) {
  const size_t stride = ((size_t)w + 31) / 32 + 2;
  // image words, the 512-entry window table, two flag words (+ pad), one "last change" byte per image word
  return ((size_t)h + 2) * stride * 4 + 512 + 16 + ((size_t)h + 2) * stride;
}

// 16 mask bytes -> 16 bits (byte k of the group -> bit k)
__device__ __forceinline__ uint32_t nonzero_bits4(uint32_t u) {
  return (uint32_t)((u & 0xffu) != 0) | ((uint32_t)((u & 0xff00u) != 0) << 1) | ((uint32_t)((u & 0xff0000u) != 0) << 2) |
         ((uint32_t)((u & 0xff000000u) != 0) << 3);
}
// 4 bits -> 4 bytes of 0 / 1 (bit k -> byte k): the four shifted copies do not overlap, so the product carries nothing
__device__ __forceinline__ uint32_t spread_bits4(uint32_t x) { return ((x & 15u) * 0x00204081u) & 0x01010101u; }

// A row of the 3 x 3 window as bits (W side, centre, E side) for every column j of a word: bit j + 1 of the returned value is
// column j of `mid`, bit 0 the last column of the word to its left, bit 33 the first column of the word to its right.
__device__ __forceinline__ uint64_t widen(uint32_t left, uint32_t mid, uint32_t right) {
  return (uint64_t)(left >> 31) | ((uint64_t)mid << 1) | ((uint64_t)(right & 1u) << 33);
}

// One sub-iteration on one non-zero word c: `img` points at it inside the bordered LDS image.
__device__ __forceinline__ uint32_t thin_word(const uint32_t* img, uint32_t c, int stride, const uint8_t* table,
                                              uint32_t phase) {
  const uint64_t ea = widen(img[-stride - 1], img[-stride], img[-stride + 1]);
  const uint64_t em = widen(img[-1], c, img[1]);
  const uint64_t eb = widen(img[stride - 1], img[stride], img[stride + 1]);
  uint32_t keep = c, todo = c;
  while (todo) {
    const int j = __builtin_ctz(todo);
    todo &= todo - 1;
    const uint32_t win = (uint32_t)((ea >> j) & 7) | ((uint32_t)((em >> j) & 7) << 3) | ((uint32_t)((eb >> j) & 7) << 6);
    if (table[win] & phase) keep &= ~(1u << j);
  }
  return keep;
}

// grid = n, block = THIN_THREADS, dynamic LDS = thin_lds_bytes(h, w).  wide: w % 32 == 0 and mask / skel 16-byte aligned --
// 16 pixels per lane on the way in and out; otherwise one pixel per lane and a ballot per 64 columns.
template <int MAXW>   // image words per thread: h * ceil(w / 32) <= MAXW * THIN_THREADS
__global__ __launch_bounds__(THIN_THREADS) void thin_lut_kernel(const uint8_t* __restrict__ mask, int h, int w,
                                                                const uint8_t* __restrict__ lut256, int max_iters,
                                                                uint8_t* __restrict__ skel, int32_t* __restrict__ iters,
                                                                int wide) {
  extern __shared__ uint32_t thin_smem[];
  const int wpr = (w + 31) >> 5, stride = wpr + 2;
  const int bordered = (h + 2) * stride;
  uint32_t* img = thin_smem;
  uint8_t* table = reinterpret_cast<uint8_t*>(thin_smem + bordered);
  volatile int* flag = reinterpret_cast<volatile int*>(thin_smem + bordered + 128);
  uint8_t* last = reinterpret_cast<uint8_t*>(thin_smem + bordered + 132);   // [bordered], indexed like img
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const size_t base = (size_t)blockIdx.x * h * w;
  const uint8_t* src = mask + base;
  uint8_t* dst = skel + base;

  for (int i = tid; i < bordered; i += THIN_THREADS) {
    img[i] = 0;
    last[i] = 255;   // "changed in sub-iteration -1": sub-iterations 0 and 1 look at every word
  }
  // window index (NW N NE | W . E | SW S SE as bits 0-2 | 3-5 | 6-8) -> the caller's table, indexed by
  // NW 1, N 2, NE 4, E 8, SE 16, S 32, SW 64, W 128
  if (tid < 512) {
    const int t = tid;
    const int code = (t & 7) | ((t >> 5 & 1) << 3) | ((t >> 8 & 1) << 4) | ((t >> 7 & 1) << 5) | ((t >> 6 & 1) << 6) |
                     ((t >> 3 & 1) << 7);
    table[t] = lut256[code];
  }
  if (tid < 2) flag[tid] = 0;
  __syncthreads();

  // ---- pack ----
  if (wide) {
    const int groups = h * wpr * 2;   // 16 pixels each; w % 32 == 0: group g is half (g & 1) of word g >> 1 in row-major order
    const uint4* src16 = reinterpret_cast<const uint4*>(src);
    for (int g0 = wave * 64; g0 < groups; g0 += THIN_THREADS) {   // (the trip count is wave-uniform: the shuffle is safe)
      const int g = g0 + lane;
      uint32_t bits = 0;
      if (g < groups) {
        const uint4 q = src16[g];
        bits = nonzero_bits4(q.x) | (nonzero_bits4(q.y) << 4) | (nonzero_bits4(q.z) << 8) | (nonzero_bits4(q.w) << 12);
      }
      const uint32_t other = __shfl_xor(bits, 1);
      if (g < groups && !(g & 1)) {
        const int wi = g >> 1, row = wi / wpr, col = wi - row * wpr;
        img[(row + 1) * stride + col + 1] = bits | (other << 16);
      }
    }
  } else {
    const int chunks = (w + 63) >> 6, items = h * chunks;
    for (int it = wave; it < items; it += THIN_THREADS / 64) {
      const int row = it / chunks, ch = it - row * chunks, col = ch * 64 + lane;
      const int on = col < w ? (src[(size_t)row * w + col] != 0) : 0;
      const unsigned long long b = __ballot(on);
      if (lane == 0) img[(row + 1) * stride + 2 * ch + 1] = (uint32_t)b;
      if (lane == 1 && 2 * ch + 1 < wpr) img[(row + 1) * stride + 2 * ch + 2] = (uint32_t)(b >> 32);
    }
  }
  __syncthreads();

  // ---- thin ----
  const int words = h * wpr;   // <= THIN_THREADS * MAXW (the host chose MAXW)
  // this thread's words tid, tid + 1024, ...: their offsets in the bordered image (< 2^14 + a border), two per register
  constexpr uint32_t NONE = 0xffffu;
  uint32_t off2[(MAXW + 1) / 2];
#pragma unroll
  for (int i = 0; i < MAXW; ++i) {
    const int k = tid + i * THIN_THREADS;
    const int row = k / wpr, col = k - row * wpr;
    const uint32_t o = k < words ? (uint32_t)((row + 1) * stride + col + 1) : NONE;
    off2[i >> 1] = (i & 1) ? (off2[i >> 1] | (o << 16)) : o;
  }
  auto off = [&](int i) -> uint32_t { return (off2[i >> 1] >> ((i & 1) * 16)) & 0xffffu; };
  // A word's new value is a function of its 3 x 3 words and the sub-iteration's parity.  last[o] is the number (mod 256) of
  // the latest sub-iteration that changed a word of o's 3 x 3: when that is more than two sub-iterations back, the word was
  // left alone two sub-iterations ago -- same parity, same 3 x 3 -- and is left alone again without being looked at.
  // (A stale byte that wraps round to "recent" only costs a look.)  Converged parts of the image cost two LDS reads per word.
  int done_at = -1;
  uint32_t sub = 0;   // sub-iterations so far
  for (int it = 1; it <= max_iters; ++it) {
    volatile int* deleted = flag + (it & 1);
#pragma unroll 1
    for (uint32_t phase = 1; phase <= 2; ++phase, ++sub) {
      uint32_t next[MAXW];
      uint32_t changed = 0;
#pragma unroll
      for (int i = 0; i < MAXW; ++i) {
        next[i] = 0;
        if (off(i) != NONE) {
          const uint32_t c = img[off(i)];
          if (c && ((sub - last[off(i)]) & 255u) <= 2u) {   // (an all-zero word: one LDS read)
            next[i] = thin_word(img + off(i), c, stride, table, phase);
            if (next[i] != c) changed |= 1u << i;
          }
        }
      }
      __syncthreads();   // every read of this sub-iteration is done
#pragma unroll
      for (int i = 0; i < MAXW; ++i)
        if (changed & (1u << i)) {
          img[off(i)] = next[i];
          uint8_t* l = last + off(i);   // (the border rows and columns of `last` take the writes of edge words)
          const uint8_t now = (uint8_t)sub;
          l[-stride - 1] = now; l[-stride] = now; l[-stride + 1] = now;
          l[-1] = now;          l[0] = now;       l[1] = now;
          l[stride - 1] = now;  l[stride] = now;  l[stride + 1] = now;
        }
      if (changed) *deleted = 1;
      if (phase == 2 && tid == 0) flag[(it + 1) & 1] = 0;   // the next iteration's word: last read one iteration ago
      __syncthreads();   // the stores are visible
    }
    if (*deleted == 0) {   // the same LDS word for every thread, read after the barrier: a uniform exit
      done_at = it;
      break;
    }
  }
  if (tid == 0) iters[blockIdx.x] = done_at;

  // ---- unpack ----
  if (wide) {
    const int groups = h * wpr * 2;
    uint4* dst16 = reinterpret_cast<uint4*>(dst);
    for (int g = tid; g < groups; g += THIN_THREADS) {
      const int wi = g >> 1, row = wi / wpr, col = wi - row * wpr;
      const uint32_t b = img[(row + 1) * stride + col + 1] >> ((g & 1) * 16);
      dst16[g] = make_uint4(spread_bits4(b), spread_bits4(b >> 4), spread_bits4(b >> 8), spread_bits4(b >> 12));
    }
  } else {
    const int chunks = (w + 63) >> 6, items = h * chunks;
    for (int it = wave; it < items; it += THIN_THREADS / 64) {
      const int row = it / chunks, ch = it - row * chunks, col = ch * 64 + lane;
      if (col < w) dst[(size_t)row * w + col] = (uint8_t)((img[(row + 1) * stride + (col >> 5) + 1] >> (col & 31)) & 1u);
    }
  }
}

// The eight neighbours of pixel (y, x) of an h x w byte image as bits: bit i = neighbour i of the walk N, NE, E, SE, S, SW, W, NW
// is on.  Neighbours outside the image are off.  (Eight independent loads; the centre is not read.)
__device__ __forceinline__ uint32_t ring_of(const uint8_t* __restrict__ s, int h, int w, int y, int x) {
  const bool up = y > 0, down = y + 1 < h, left = x > 0, right = x + 1 < w;
  const uint8_t* p = s + (size_t)y * w + x;
  uint32_t ring = 0;
  ring |= (uint32_t)(up && p[-w] != 0) << 0;
  ring |= (uint32_t)(up && right && p[-w + 1] != 0) << 1;
  ring |= (uint32_t)(right && p[1] != 0) << 2;
  ring |= (uint32_t)(down && right && p[w + 1] != 0) << 3;
  ring |= (uint32_t)(down && p[w] != 0) << 4;
  ring |= (uint32_t)(down && left && p[w - 1] != 0) << 5;
  ring |= (uint32_t)(left && p[-1] != 0) << 6;
  ring |= (uint32_t)(up && left && p[-w - 1] != 0) << 7;
  return ring;
}

// A(p) from the ring of an ON pixel, or 0 when it is not a node
__device__ __forceinline__ int class_of_ring(uint32_t ring) {
  const uint32_t following = ((ring >> 1) | (ring << 7)) & 0xffu;   // bit i = neighbour i + 1 (the walk closes on N)
  const int a = __builtin_popcount(~ring & following & 0xffu);
  return (a == 1 || a >= 3) ? a : 0;
}

// A(p) of pixel (y, x), or 0 when the pixel is off or not a node
__device__ __forceinline__ int node_class_of(const uint8_t* __restrict__ s, int h, int w, int y, int x) {
  return s[(size_t)y * w + x] ? class_of_ring(ring_of(s, h, w, y, x)) : 0;
}

// grid = n, block = NODE_THREADS
__global__ __launch_bounds__(NODE_THREADS) void skel_nodes_kernel(const uint8_t* __restrict__ skel, int h, int w,
                                                                  uint8_t* __restrict__ node_class,
                                                                  int32_t* __restrict__ coords, int cap,
                                                                  int32_t* __restrict__ counts) {
  constexpr int WAVES = NODE_THREADS / 64;
  constexpr int U = 8, STEP = U * 64;   // pixels per wave step: eight centre bytes per lane in flight, then their neighbours
  constexpr int KEEP = 256;      // a wave remembers this many of its nodes for the second walk
  __shared__ int wave_nodes[WAVES];
  __shared__ int found[WAVES][KEEP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int total = h * w;   // <= 2^30 (checked by the host)
  const uint8_t* s = skel + (size_t)blockIdx.x * total;
  uint8_t* nc = node_class ? node_class + (size_t)blockIdx.x * total : nullptr;
  const int per = (((total + WAVES - 1) / WAVES) + STEP - 1) / STEP * STEP;   // a wave's stretch: whole steps
  const int begin = min(total, wave * per), end = min(total, begin + per);
  const unsigned long long below = (1ull << lane) - 1ull;

  int mine = 0;   // wave-uniform
  for (int p0 = begin; p0 < end; p0 += STEP) {
    uint8_t centre[U];
    uint32_t ring[U];
    uint32_t any = 0;
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * 64 + lane;
      centre[u] = p < end ? s[p] : (uint8_t)0;
      any |= centre[u];
      ring[u] = 0;
    }
    if (__ballot(any != 0)) {   // wave-uniform; the neighbours of all eight pixels are loaded together, on or off
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int p = p0 + u * 64 + lane;
        if (p < end) {
          const int y = p / w;
          ring[u] = ring_of(s, h, w, y, p - y * w);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int p = p0 + u * 64 + lane;
      const int a = centre[u] ? class_of_ring(ring[u]) : 0;
      if (nc && p < end) nc[p] = (uint8_t)a;
      const unsigned long long b = __ballot(a != 0);
      if (a) {
        const int k = mine + __builtin_popcountll(b & below);
        if (k < KEEP) found[wave][k] = p;
      }
      mine += __builtin_popcountll(b);
    }
  }
  if (lane == 0) wave_nodes[wave] = mine;
  __syncthreads();
  int before = 0, all = 0;
#pragma unroll
  for (int i = 0; i < WAVES; ++i) {
    const int c = wave_nodes[i];
    before += i < wave ? c : 0;
    all += c;
  }
  if (tid == 0) counts[blockIdx.x] = all;
  if (cap <= 0) return;

  int32_t* out = coords + (size_t)blockIdx.x * cap * 2;
  if (mine <= KEEP) {   // the usual case: the wave's nodes are in LDS, in order
    for (int k = lane; k < mine && before + k < cap; k += 64) {
      const int p = found[wave][k], y = p / w;
      out[2 * (size_t)(before + k)] = y;
      out[2 * (size_t)(before + k) + 1] = p - y * w;
    }
    return;
  }
  int running = before;   // wave-uniform
  for (int p0 = begin; p0 < end && running < cap; p0 += 64) {   // (an image dense with nodes: walk the stretch again)
    const int p = p0 + lane;
    int a = 0, y = 0, x = 0;
    if (p < end) {
      y = p / w;
      x = p - y * w;
      a = node_class_of(s, h, w, y, x);
    }
    const unsigned long long b = __ballot(a != 0);
    if (a) {
      const int pos = running + __builtin_popcountll(b & below);
      if (pos < cap) {
        out[2 * (size_t)pos] = y;
        out[2 * (size_t)pos + 1] = x;
      }
    }
    running += __builtin_popcountll(b);
  }
}

}  // namespace dsg

DSG_API int dsg_thin_lut_u8(const uint8_t* mask, int32_t n, int32_t h, int32_t w, const uint8_t* lut256, int32_t max_iters,
                            uint8_t* skel, int32_t* iters, void* stream) {
  DSG_CHECK_ARG(mask && lut256 && skel && iters, "dsg_thin_lut_u8: NULL pointer");
  DSG_CHECK_ARG(mask != skel, "dsg_thin_lut_u8: skel must not alias mask");
  DSG_CHECK_ARG(n > 0 && h > 0 && w > 0 && max_iters > 0, "dsg_thin_lut_u8: bad dims (n=%d h=%d w=%d max_iters=%d)", n, h, w,
                max_iters);
  // (an image inside the LDS limit has fewer than 12.6 K words: THIN_THREADS * THIN_MAX_WORDS holds them; checked all the same)
  const int64_t words = (int64_t)h * (((int64_t)w + 31) / 32);
  DSG_CHECK_ARG(dsg::thin_lds_bytes(h, w) <= dsg::THIN_LDS_MAX && words <= (int64_t)dsg::THIN_THREADS * dsg::THIN_MAX_WORDS,
                "dsg_thin_lut_u8: a %d x %d image does not fit one workgroup's LDS (bit-packed with its border: %zu bytes, "
                "limit %zu)", h, w, dsg::thin_lds_bytes(h, w), dsg::THIN_LDS_MAX);
  const int wide = w % 32 == 0 && reinterpret_cast<uintptr_t>(mask) % 16 == 0 && reinterpret_cast<uintptr_t>(skel) % 16 == 0;
  const auto kernel = words <= 4 * dsg::THIN_THREADS   ? dsg::thin_lut_kernel<4>     // up to 256 x 512
                      : words <= 8 * dsg::THIN_THREADS ? dsg::thin_lut_kernel<8>     // up to 512 x 512
                                                       : dsg::thin_lut_kernel<dsg::THIN_MAX_WORDS>;
  hipLaunchKernelGGL(kernel, dim3(n), dim3(dsg::THIN_THREADS), dsg::thin_lds_bytes(h, w), static_cast<hipStream_t>(stream),
                     mask, h, w, lut256, max_iters, skel, iters, wide);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_skel_nodes_u8(const uint8_t* skel, int32_t n, int32_t h, int32_t w, uint8_t* node_class, int32_t* coords,
                              int32_t cap, int32_t* counts, void* stream) {
  DSG_CHECK_ARG(skel && counts, "dsg_skel_nodes_u8: NULL pointer");
  DSG_CHECK_ARG(n > 0 && h > 0 && w > 0 && (int64_t)h * w <= (1 << 30), "dsg_skel_nodes_u8: bad dims (n=%d h=%d w=%d)", n, h, w);
  DSG_CHECK_ARG(cap >= 0 && (cap == 0 || coords), "dsg_skel_nodes_u8: cap=%d needs a coords buffer", cap);
  DSG_CHECK_ARG(node_class != skel, "dsg_skel_nodes_u8: node_class must not alias skel");
  hipLaunchKernelGGL(dsg::skel_nodes_kernel, dim3(n), dim3(dsg::NODE_THREADS), 0, static_cast<hipStream_t>(stream), skel, h,
                     w, node_class, coords, cap, counts);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}
