// Connected components (continued): the primitive both halves of the vectoriser need next.
// find_dense_skeleton_nodes / add_dense_nodes (DriveSceneGen/vectorization/graph/extract_network.py:96-122, called at
// :241-242) label the 2 x 2-eroded skeleton with scipy.ndimage.label and take each component's centre of mass;
// extract_agents (vectorization/direct/extract_vehicles.py:147-148) looks for the blobs of its thresholded channel.
//
// Labelling is union-find on the label array itself, integer arithmetic only: a zero fill of the error words and six launches,
// no hand-off inside any of them.
//
//  ccl_tile_kernel     One workgroup per TILE_H x TILE_W tile, one pixel per thread.  The mask is read here (and only here), with
//                      the 2 x 2 erosion folded into the read.  Label equivalence in LDS (Hawick, Leist & Playne, Parallel
//                      Computing 36(12), 2010): a pixel's label starts as its own index in the tile, a pass lowers the root of
//                      every pixel that has a neighbour with a smaller label (LDS atomicMin) and then points every pixel at
//                      its root; passes repeat until one changes nothing.  Out: the parent of every on pixel = the tile-local
//                      minimum GLOBAL linear index of its component.
//  ccl_merge_kernel    One wave per tile: the pixels of its first row and first column are united with their neighbours in the
//                      tiles above and to the left.  union(a, b): find both roots, atomicMin the smaller into the larger's
//                      word, and continue from what the atomic returned whenever the larger was no longer a root.  A root is
//                      always the smallest index of its tree, so the forest after the last union is the same whatever the
//                      order the unions ran in.  Every load of another workgroup's words is a relaxed agent-scope atomic load
//                      (no stale L1 line can be read); a value that is old all the same is an earlier, larger ancestor of the
//                      same component -- the loops only ever walk to smaller indices.
//  ccl_flatten_kernel  Points every pixel at its root and counts the roots of every CHUNK of the row-major order.
//  ccl_scan_kernel     One workgroup per image: exclusive scan of the chunk counts, counts[i].
//  ccl_rank_kernel     A root's label = the roots before its chunk + its rank inside the chunk (ballot + popcount) + 1: scipy's
//                      numbering, components in row-major order of their first pixel.  Fixed by counts and a scan, never by the
//                      arrival order of atomics.
//  ccl_resolve_kernel  Every other on pixel copies its root's label.
//
// While the forest is being built a word of `labels` holds ~parent (negative) for an on pixel and 0 for an off one; labels are
// positive, so the three states never mix and the array needs no companion.  atomicMin on parents is atomicMax on these words.
// Every walk moves to a strictly smaller index, and is cut after h * w steps all the same: a cut sets the image's error word and
// counts[i] = -1.
//
//  cc_stats_kernel     area, bounding box and the five coordinate sums per label.  A wave reads 64 pixels of one row; the first
//                      lane of every run of equal labels adds the whole run in closed form -- into a small per-workgroup table
//                      in LDS, which is added to memory at the end with one atomic set per label and workgroup (a run whose
//                      slot is taken by another label goes to memory directly).  All sums are integers: the result does not
//                      depend on the order of the atomics.
//  cc_centers_kernel   (sum_r / area, sum_c / area).
//  merge_nodes_kernel  add_dense_nodes: one workgroup per image, kept dense nodes appended in the dense list's order (scan).
#include <climits>
#include "dsg_common.h"

namespace dsg {

constexpr int CCL_TILE_H = 32, CCL_TILE_W = 32;
constexpr int CCL_TILE_THREADS = CCL_TILE_H * CCL_TILE_W;   // one pixel per thread
constexpr int CCL_CHUNK_THREADS = 256, CCL_CHUNK_ITERS = 4;
constexpr int CCL_CHUNK = CCL_CHUNK_THREADS * CCL_CHUNK_ITERS;   // pixels per chunk of the row-major order
constexpr int64_t CCL_MAX_PIXELS = (int64_t)1 << 30;
constexpr int STAT_ROWS = 16, STAT_COLS = 64, STAT_THREADS = 256, STAT_SLOTS = 128;
constexpr int MERGE_NODES_THREADS = 256;

static inline bool overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  if (!a || !b) return false;
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y ? y - x < abytes : x - y < bbytes;
}

__device__ __forceinline__ int ld_agent(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_agent(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ---- 1: tiles -----------------------------------------------------------------------------------------------------------------
// grid = (tiles_x * tiles_y, n), block = CCL_TILE_THREADS
__global__ __launch_bounds__(CCL_TILE_THREADS) void ccl_tile_kernel(const uint8_t* __restrict__ mask, int h, int w, int tiles_x,
                                                                    int eight, int erode, int32_t* __restrict__ labels,
                                                                    int32_t* __restrict__ err) {
  constexpr int TW = CCL_TILE_W, TH = CCL_TILE_H, STRIDE = TW + 2, OFF = INT_MAX;
  __shared__ int lab[(TH + 2) * STRIDE];   // the tile inside a one-pixel border of OFF: neighbours are read without an edge test
  __shared__ int changed;
  const int tid = threadIdx.x, lx = tid % TW, ly = tid / TW;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int y = ty * TH + ly, x = tx * TW + lx;
  const size_t base = (size_t)blockIdx.y * h * w;
  const uint8_t* m = mask + base;

  bool on = false;
  if (y < h && x < w) {
    const size_t p = (size_t)y * w + x;
    on = m[p] != 0;
    // erosion by a 2 x 2 block anchored at the larger indices: (y-1..y) x (x-1..x) all on and inside the image
    if (erode) on = on && y > 0 && x > 0 && m[p - 1] != 0 && m[p - w] != 0 && m[p - w - 1] != 0;
  }
  for (int i = tid; i < (TH + 2) * STRIDE; i += CCL_TILE_THREADS) lab[i] = OFF;
  __syncthreads();
  const int me = (ly + 1) * STRIDE + lx + 1;
  if (on) lab[me] = tid;
  auto cell = [&](int l) { return (l / TW + 1) * STRIDE + l % TW + 1; };   // where the pixel with local index l lives
  volatile int* vlab = lab;

  bool converged = false;
  for (int pass = 0; pass < CCL_TILE_THREADS; ++pass) {   // (a pass that changes something lowers a label: it ends; cut anyway)
    if (tid == 0) changed = 0;
    __syncthreads();
    if (on) {
      const int cur = lab[me];   // a root: the previous pass pointed every pixel at one
      int lo = min(min(lab[me - 1], lab[me + 1]), min(lab[me - STRIDE], lab[me + STRIDE]));
      if (eight)
        lo = min(lo, min(min(lab[me - STRIDE - 1], lab[me - STRIDE + 1]), min(lab[me + STRIDE - 1], lab[me + STRIDE + 1])));
      if (lo < cur) {
        atomicMin(&lab[cell(cur)], lo);
        changed = 1;
      }
    }
    __syncthreads();
    if (on) {
      // to the root: every step reads a smaller label (a word another thread lowers meanwhile only shortens the walk)
      int l = vlab[me], up = vlab[cell(l)];
      while (up != l) {
        l = up;
        up = vlab[cell(l)];
      }
      vlab[me] = l;
    }
    const int again = *(volatile int*)&changed;   // written before the barrier above, cleared after the one below: uniform
    __syncthreads();
    if (!again) {
      converged = true;
      break;
    }
  }
  if (!converged && tid == 0) err[blockIdx.y] = 1;
  if (y < h && x < w) {
    int32_t v = 0;
    if (on) {
      const int l = lab[me];
      v = ~(int32_t)((ty * TH + l / TW) * w + tx * TW + l % TW);   // < 2^30
    }
    labels[base + (size_t)y * w + x] = v;
  }
}

// ---- 2: tile borders ----------------------------------------------------------------------------------------------------------
// the root of pixel a (>= 0) of image L, or -1 after `limit` steps
__device__ __forceinline__ int ccl_find(const int32_t* L, int a, int limit) {
  for (int steps = 0; steps <= limit; ++steps) {
    const int up = ~ld_agent(L + a);   // (an on pixel: the word is ~parent)
    if (up == a) return a;
    if (up < 0) return -1;   // (the word of an off pixel: never a parent in a forest this file built)
    a = up;                  // up < a
  }
  return -1;
}

__device__ __forceinline__ bool ccl_union(int32_t* L, int a, int b, int limit) {
  a = ccl_find(L, a, limit);
  b = ccl_find(L, b, limit);
  if (a < 0 || b < 0) return false;
  for (int steps = 0; steps <= limit; ++steps) {
    if (a == b) return true;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    // a > b: hang a below b if it is (still) a root.  The word held ~old with old <= a.
    const int old = ~atomicMax(L + a, ~b);
    if (old == a) return true;
    a = old;   // a had been given the parent old < a meanwhile: old and b are what is left to unite
  }
  return false;
}

// grid = (tiles_x * tiles_y, n), block = CCL_TILE_W + CCL_TILE_H: lane t < TILE_W is pixel (0, t) of the tile and looks up
// (N, and NW / NE with `eight`), the others are pixel (t - TILE_W, 0) and look left (W, and NW / SW).  Every pair of adjacent pixels
// in two different tiles is met by one of them (the tile's corner pixel by both: a union is idempotent).
__global__ __launch_bounds__(CCL_TILE_W + CCL_TILE_H) void ccl_merge_kernel(int h, int w, int tiles_x, int eight,
                                                                            int32_t* __restrict__ labels,
                                                                            int32_t* __restrict__ err) {
  const int t = threadIdx.x;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const bool top = t < CCL_TILE_W;
  const int y = ty * CCL_TILE_H + (top ? 0 : t - CCL_TILE_W), x = tx * CCL_TILE_W + (top ? t : 0);
  if (y >= h || x >= w || (top ? ty == 0 : tx == 0)) return;
  int32_t* L = labels + (size_t)blockIdx.y * h * w;
  const int limit = h * w, p = y * w + x;
  if (ld_agent(L + p) == 0) return;
  bool ok = true;
  for (int k = -1; k <= 1; ++k) {
    if (k != 0 && !eight) continue;
    const int qy = top ? y - 1 : y + k, qx = top ? x + k : x - 1;
    if (qy < 0 || qy >= h || qx < 0 || qx >= w) continue;
    const int q = qy * w + qx;
    if (ld_agent(L + q) != 0) ok = ccl_union(L, p, q, limit) && ok;
  }
  if (!ok) err[blockIdx.y] = 1;
}

// ---- 3: flatten, count roots per chunk ------------------------------------------------------------------------------------------
// grid = (chunks, n), block = CCL_CHUNK_THREADS.  Pixel of (iteration k, thread t) = chunk * CCL_CHUNK + k * CCL_CHUNK_THREADS + t.
__global__ __launch_bounds__(CCL_CHUNK_THREADS) void ccl_flatten_kernel(int total, int chunks, int32_t* __restrict__ labels,
                                                                        int32_t* __restrict__ chunk_roots,
                                                                        int32_t* __restrict__ err) {
  __shared__ int wave_roots[CCL_CHUNK_THREADS / 64];
  int32_t* L = labels + (size_t)blockIdx.y * total;
  const int tid = threadIdx.x;
  int roots = 0;   // wave-uniform
  bool ok = true;
  for (int k = 0; k < CCL_CHUNK_ITERS; ++k) {
    const int p = blockIdx.x * CCL_CHUNK + k * CCL_CHUNK_THREADS + tid;   // chunks * CCL_CHUNK < 2^30 + 2^10
    bool root = false;
    if (p < total) {
      const int v = ld_agent(L + p);
      if (v != 0) {
        const int first = ~v;
        root = first == p;
        if (!root) {
          const int r = ccl_find(L, first, total);
          if (r < 0) {
            ok = false;
          } else if (r != first) {
            // (other workgroups walk through these words meanwhile: they read ~first or ~r, both ancestors)
            st_agent(L + p, ~r);
            st_agent(L + first, ~r);   // p's tile root: the rest of the tile then finds r in one step
          }
        }
      }
    }
    roots += __builtin_popcountll(__ballot(root));
  }
  if (!ok) err[blockIdx.y] = 1;
  if ((tid & 63) == 0) wave_roots[tid >> 6] = roots;
  __syncthreads();
  if (tid == 0) {
    int all = 0;
    for (int i = 0; i < CCL_CHUNK_THREADS / 64; ++i) all += wave_roots[i];
    chunk_roots[(size_t)blockIdx.y * chunks + blockIdx.x] = all;
  }
}

// ---- 4: scan ------------------------------------------------------------------------------------------------------------------
// grid = n, block = CCL_CHUNK_THREADS: chunk_roots[i][.] -> its exclusive prefix sums, counts[i]
__global__ __launch_bounds__(CCL_CHUNK_THREADS) void ccl_scan_kernel(int chunks, int32_t* __restrict__ chunk_roots,
                                                                     const int32_t* __restrict__ err,
                                                                     int32_t* __restrict__ counts) {
  constexpr int WAVES = CCL_CHUNK_THREADS / 64;
  __shared__ int wave_sum[WAVES];
  int32_t* c = chunk_roots + (size_t)blockIdx.x * chunks;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int carry = 0;   // uniform
  for (int j0 = 0; j0 < chunks; j0 += CCL_CHUNK_THREADS) {
    const int j = j0 + tid;
    const int v = j < chunks ? c[j] : 0;
    int incl = v;
    for (int d = 1; d < 64; d <<= 1) {
      const int o = __shfl_up(incl, d);
      if (lane >= d) incl += o;
    }
    if (lane == 63) wave_sum[wave] = incl;
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < WAVES; ++i) {
      before += i < wave ? wave_sum[i] : 0;
      all += wave_sum[i];
    }
    if (j < chunks) c[j] = carry + before + incl - v;
    carry += all;
    __syncthreads();   // wave_sum is rewritten by the next round
  }
  if (tid == 0) counts[blockIdx.x] = err[blockIdx.x] ? -1 : carry;
}

// ---- 5: number the roots --------------------------------------------------------------------------------------------------------
// grid = (chunks, n), block = CCL_CHUNK_THREADS; the chunk layout of ccl_flatten_kernel
__global__ __launch_bounds__(CCL_CHUNK_THREADS) void ccl_rank_kernel(int total, int chunks, int32_t* __restrict__ labels,
                                                                     const int32_t* __restrict__ chunk_base) {
  constexpr int WAVES = CCL_CHUNK_THREADS / 64;
  __shared__ int part[CCL_CHUNK_ITERS][WAVES];
  int32_t* L = labels + (size_t)blockIdx.y * total;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  bool root[CCL_CHUNK_ITERS];
  int rank[CCL_CHUNK_ITERS];
#pragma unroll
  for (int k = 0; k < CCL_CHUNK_ITERS; ++k) {
    const int p = blockIdx.x * CCL_CHUNK + k * CCL_CHUNK_THREADS + tid;
    root[k] = p < total && L[p] == ~p;
    const unsigned long long b = __ballot(root[k]);
    rank[k] = __builtin_popcountll(b & below);
    if (lane == 0) part[k][wave] = __builtin_popcountll(b);
  }
  __syncthreads();
  const int base = chunk_base[(size_t)blockIdx.y * chunks + blockIdx.x];
  int before = 0;   // the roots of the (iteration, wave) pairs in front of this one, in pixel order
#pragma unroll
  for (int k = 0; k < CCL_CHUNK_ITERS; ++k) {
#pragma unroll
    for (int i = 0; i < WAVES; ++i) {
      if (i == wave && root[k]) L[blockIdx.x * CCL_CHUNK + k * CCL_CHUNK_THREADS + tid] = base + before + rank[k] + 1;
      before += part[k][i];
    }
  }
}

// ---- 6: everything else takes its root's number ---------------------------------------------------------------------------------
// grid = (chunks, n), block = CCL_CHUNK_THREADS.  Reads only words that are positive (roots: written by the launch before, by
// nobody here) and its own.
__global__ __launch_bounds__(CCL_CHUNK_THREADS) void ccl_resolve_kernel(int total, int32_t* __restrict__ labels) {
  int32_t* L = labels + (size_t)blockIdx.y * total;
  for (int k = 0; k < CCL_CHUNK_ITERS; ++k) {
    const int p = blockIdx.x * CCL_CHUNK + k * CCL_CHUNK_THREADS + threadIdx.x;
    if (p < total) {
      const int v = L[p];
      if (v < 0) {
        const int r = L[~v];
        L[p] = r > 0 ? r : 0;   // (r <= 0 only after a cut walk, counts[i] = -1: keep the array free of parent words)
      }
    }
  }
}

// ---- statistics ---------------------------------------------------------------------------------------------------------------
__global__ void cc_stats_init_kernel(const int32_t* __restrict__ counts, int cap, dsg_cc_stat* __restrict__ stats) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= min(counts[blockIdx.y], cap)) return;   // (counts = -1: nothing)
  dsg_cc_stat s;
  s.area = 0;
  s.r0 = INT_MAX;
  s.c0 = INT_MAX;
  s.r1 = 0;
  s.c1 = 0;
  s.reserved = 0;
  s.sum_r = s.sum_c = s.sum_rr = s.sum_cc = s.sum_rc = 0;
  stats[(size_t)blockIdx.y * cap + k] = s;
}

struct cc_run {   // `len` pixels of row r from column c on
  int len, r, c;
  __device__ long long sum_c() const { return (long long)len * c + (long long)len * (len - 1) / 2; }
  __device__ long long sum_cc() const {
    const long long n = len;
    return n * c * c + (long long)c * n * (n - 1) + (n - 1) * n * (2 * n - 1) / 6;
  }
};

__device__ __forceinline__ void add64(long long* p, long long v) {
  atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// one set of atomics for `area` pixels with these extents and sums (LDS or memory)
__device__ __forceinline__ void cc_add(dsg_cc_stat* s, int area, int r0, int c0, int r1, int c1, long long sr, long long sc,
                                       long long srr, long long scc, long long src) {
  atomicAdd(&s->area, area);
  atomicMin(&s->r0, r0);
  atomicMin(&s->c0, c0);
  atomicMax(&s->r1, r1);
  atomicMax(&s->c1, c1);
  add64(reinterpret_cast<long long*>(&s->sum_r), sr);
  add64(reinterpret_cast<long long*>(&s->sum_c), sc);
  add64(reinterpret_cast<long long*>(&s->sum_rr), srr);
  add64(reinterpret_cast<long long*>(&s->sum_cc), scc);
  add64(reinterpret_cast<long long*>(&s->sum_rc), src);
}

// grid = (tiles_x * tiles_y, n) of STAT_ROWS x STAT_COLS tiles, block = STAT_THREADS: wave v reads rows v, v + 4, ... of the tile
__global__ __launch_bounds__(STAT_THREADS) void cc_stats_kernel(const int32_t* __restrict__ labels, int h, int w, int tiles_x,
                                                                const int32_t* __restrict__ counts, int cap,
                                                                dsg_cc_stat* __restrict__ stats) {
  __shared__ dsg_cc_stat slot[STAT_SLOTS];
  __shared__ int owner[STAT_SLOTS];   // the label a slot belongs to, 0 = free
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int top = min(counts[blockIdx.y], cap);   // labels 1..top have a record
  if (top <= 0) return;   // (uniform)
  const int32_t* L = labels + (size_t)blockIdx.y * h * w;
  dsg_cc_stat* out = stats + (size_t)blockIdx.y * cap;
  for (int i = tid; i < STAT_SLOTS; i += STAT_THREADS) {
    owner[i] = 0;
    slot[i].area = 0;
    slot[i].r0 = INT_MAX;
    slot[i].c0 = INT_MAX;
    slot[i].r1 = 0;
    slot[i].c1 = 0;
    slot[i].sum_r = slot[i].sum_c = slot[i].sum_rr = slot[i].sum_cc = slot[i].sum_rc = 0;
  }
  __syncthreads();
  const int x = tx * STAT_COLS + lane;
  for (int ry = wave; ry < STAT_ROWS; ry += STAT_THREADS / 64) {
    const int y = ty * STAT_ROWS + ry;
    if (y >= h) break;   // (wave-uniform)
    int l = x < w ? L[(size_t)y * w + x] : 0;
    if (l > top) l = 0;
    const int left = __shfl_up(l, 1);
    const bool head = l > 0 && (lane == 0 || left != l);
    // the run ends in front of the next lane whose label differs from its left neighbour's (or at the wave's end)
    const unsigned long long edges = __ballot(lane == 0 || left != l);
    if (head) {
      const unsigned long long later = lane == 63 ? 0ull : edges >> (lane + 1);
      const cc_run run = {later ? __builtin_ctzll(later) + 1 : 64 - lane, y, x};
      const long long sc = run.sum_c();
      const int s = l & (STAT_SLOTS - 1);
      const int was = atomicCAS(&owner[s], 0, l);
      dsg_cc_stat* dst = (was == 0 || was == l) ? &slot[s] : &out[l - 1];
      cc_add(dst, run.len, y, x, y + 1, x + run.len, (long long)run.len * y, sc, (long long)run.len * y * y, run.sum_cc(),
             (long long)y * sc);
    }
  }
  __syncthreads();
  for (int i = tid; i < STAT_SLOTS; i += STAT_THREADS)
    if (owner[i]) {
      const dsg_cc_stat& s = slot[i];
      cc_add(&out[owner[i] - 1], s.area, s.r0, s.c0, s.r1, s.c1, s.sum_r, s.sum_c, s.sum_rr, s.sum_cc, s.sum_rc);
    }
}

__global__ void cc_centers_kernel(const dsg_cc_stat* __restrict__ stats, const int32_t* __restrict__ counts, int cap,
                                  int32_t* __restrict__ coords) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= min(counts[blockIdx.y], cap)) return;
  const dsg_cc_stat& s = stats[(size_t)blockIdx.y * cap + k];
  int32_t* o = coords + ((size_t)blockIdx.y * cap + k) * 2;
  o[0] = (int32_t)(s.sum_r / s.area);   // area >= 1: the label exists
  o[1] = (int32_t)(s.sum_c / s.area);
}

// ---- add_dense_nodes ------------------------------------------------------------------------------------------------------------
// grid = n, block = MERGE_NODES_THREADS
__global__ __launch_bounds__(MERGE_NODES_THREADS) void merge_nodes_kernel(int32_t* __restrict__ nodes,
                                                                          const int32_t* __restrict__ counts, int cap,
                                                                          const int32_t* __restrict__ dense,
                                                                          const int32_t* __restrict__ dense_counts, int dense_cap,
                                                                          long long min_d2, int32_t* __restrict__ out_counts) {
  constexpr int WAVES = MERGE_NODES_THREADS / 64;
  __shared__ int wave_kept[WAVES];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int count = counts[blockIdx.x];
  const int listed = max(0, min(count, cap)), nd = max(0, min(dense_counts[blockIdx.x], dense_cap));
  int32_t* mine = nodes + (size_t)blockIdx.x * cap * 2;
  const int32_t* d = dense + (size_t)blockIdx.x * dense_cap * 2;
  const unsigned long long below = (1ull << lane) - 1ull;
  int kept = 0;   // uniform
  for (int j0 = 0; j0 < nd; j0 += MERGE_NODES_THREADS) {
    const int j = j0 + tid;
    bool keep = j < nd;
    int dr = 0, dc = 0;
    if (keep) {
      dr = d[2 * j];
      dc = d[2 * j + 1];
      for (int i = 0; i < listed; ++i) {   // (rows below `listed`: the original nodes, never written here)
        const long long a = (long long)mine[2 * i] - dr, b = (long long)mine[2 * i + 1] - dc;
        if (a * a + b * b < min_d2) {
          keep = false;
          break;
        }
      }
    }
    const unsigned long long b = __ballot(keep);
    if (lane == 0) wave_kept[wave] = __builtin_popcountll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int i = 0; i < WAVES; ++i) {
      before += i < wave ? wave_kept[i] : 0;
      all += wave_kept[i];
    }
    const int at = listed + kept + before + __builtin_popcountll(b & below);
    if (keep && at < cap) {
      mine[2 * (size_t)at] = dr;
      mine[2 * (size_t)at + 1] = dc;
    }
    kept += all;
    __syncthreads();
  }
  if (tid == 0) out_counts[blockIdx.x] = count + kept;
}

static inline int ccl_chunks(int64_t total) { return (int)((total + CCL_CHUNK - 1) / CCL_CHUNK); }
static inline size_t ccl_ws_bytes(int n, int64_t total) { return ((size_t)n + (size_t)n * ccl_chunks(total)) * sizeof(int32_t); }

}  // namespace dsg

DSG_API int dsg_ccl_tile_shape(int32_t* tile_h, int32_t* tile_w) {
  DSG_CHECK_ARG(tile_h && tile_w, "dsg_ccl_tile_shape: NULL pointer");
  *tile_h = dsg::CCL_TILE_H;
  *tile_w = dsg::CCL_TILE_W;
  return DSG_OK;
}

DSG_API int dsg_ccl_workspace_bytes(int32_t n, int32_t h, int32_t w, size_t* bytes) {
  DSG_CHECK_ARG(bytes, "dsg_ccl_workspace_bytes: NULL pointer");
  DSG_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w <= dsg::CCL_MAX_PIXELS,
                "dsg_ccl_workspace_bytes: bad dims (n=%d h=%d w=%d; n <= 65535, h * w <= 2^30)", n, h, w);
  *bytes = dsg::ccl_ws_bytes(n, (int64_t)h * w);
  return DSG_OK;
}

DSG_API int dsg_ccl_u8(const uint8_t* mask, int32_t n, int32_t h, int32_t w, int32_t connectivity, int32_t erode2x2,
                       int32_t* labels, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream) {
  DSG_CHECK_ARG(mask && labels && counts && workspace, "dsg_ccl_u8: NULL pointer");
  DSG_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w <= dsg::CCL_MAX_PIXELS,
                "dsg_ccl_u8: bad dims (n=%d h=%d w=%d; n <= 65535, h * w <= 2^30)", n, h, w);
  DSG_CHECK_ARG(connectivity == 1 || connectivity == 2, "dsg_ccl_u8: connectivity=%d is neither 1 (4 neighbours) nor 2 (8)",
                connectivity);
  DSG_CHECK_ARG(erode2x2 == 0 || erode2x2 == 1, "dsg_ccl_u8: erode2x2=%d is neither 0 nor 1", erode2x2);
  const int total = h * w;
  const size_t need = dsg::ccl_ws_bytes(n, total);
  if (workspace_bytes < need)
    return dsg::fail(DSG_ERR_WORKSPACE_TOO_SMALL, "dsg_ccl_u8: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  DSG_CHECK_ARG((reinterpret_cast<uintptr_t>(workspace) & 3u) == 0, "dsg_ccl_u8: workspace is not 4-byte aligned");
  const uint64_t mask_bytes = (uint64_t)n * total, label_bytes = mask_bytes * 4, count_bytes = (uint64_t)n * 4;
  DSG_CHECK_ARG(!dsg::overlap(labels, label_bytes, mask, mask_bytes), "dsg_ccl_u8: labels overlaps the mask");
  DSG_CHECK_ARG(!dsg::overlap(counts, count_bytes, mask, mask_bytes), "dsg_ccl_u8: counts overlaps the mask");
  DSG_CHECK_ARG(!dsg::overlap(workspace, need, mask, mask_bytes), "dsg_ccl_u8: the workspace overlaps the mask");
  DSG_CHECK_ARG(!dsg::overlap(labels, label_bytes, counts, count_bytes), "dsg_ccl_u8: labels overlaps counts");
  DSG_CHECK_ARG(!dsg::overlap(workspace, need, labels, label_bytes), "dsg_ccl_u8: the workspace overlaps labels");
  DSG_CHECK_ARG(!dsg::overlap(workspace, need, counts, count_bytes), "dsg_ccl_u8: the workspace overlaps counts");

  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* err = static_cast<int32_t*>(workspace);   // [n]
  int32_t* chunk_roots = err + n;                    // [n][chunks]
  const int tiles_x = dsg::cdiv(w, dsg::CCL_TILE_W), tiles_y = dsg::cdiv(h, dsg::CCL_TILE_H);   // tiles_x * tiles_y <= 2^25 + ...
  const int chunks = dsg::ccl_chunks(total), eight = connectivity == 2;
  const dim3 tiles((unsigned)((int64_t)tiles_x * tiles_y), n), by_chunk(chunks, n);
  DSG_HIP(dsg::zero_words(err, (size_t)n, st));   // (a kernel, not a memset node: see dsg_common.h)
  hipLaunchKernelGGL(dsg::ccl_tile_kernel, tiles, dim3(dsg::CCL_TILE_THREADS), 0, st, mask, h, w, tiles_x, eight, erode2x2,
                     labels, err);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsg::ccl_merge_kernel, tiles, dim3(dsg::CCL_TILE_W + dsg::CCL_TILE_H), 0, st, h, w, tiles_x, eight, labels,
                     err);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsg::ccl_flatten_kernel, by_chunk, dim3(dsg::CCL_CHUNK_THREADS), 0, st, total, chunks, labels, chunk_roots,
                     err);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsg::ccl_scan_kernel, dim3(n), dim3(dsg::CCL_CHUNK_THREADS), 0, st, chunks, chunk_roots, err, counts);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsg::ccl_rank_kernel, by_chunk, dim3(dsg::CCL_CHUNK_THREADS), 0, st, total, chunks, labels, chunk_roots);
  DSG_LAUNCH_CHECK();
  hipLaunchKernelGGL(dsg::ccl_resolve_kernel, by_chunk, dim3(dsg::CCL_CHUNK_THREADS), 0, st, total, labels);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_cc_stats_i32(const int32_t* labels, int32_t n, int32_t h, int32_t w, const int32_t* counts, dsg_cc_stat* stats,
                             int32_t cap, void* stream) {
  DSG_CHECK_ARG(labels && counts, "dsg_cc_stats_i32: NULL pointer");
  DSG_CHECK_ARG(n > 0 && n <= 65535 && h > 0 && w > 0 && (int64_t)h * w <= dsg::CCL_MAX_PIXELS && h <= 32768 && w <= 32768,
                "dsg_cc_stats_i32: bad dims (n=%d h=%d w=%d; n <= 65535, h * w <= 2^30, h and w <= 2^15)", n, h, w);
  DSG_CHECK_ARG(cap >= 0 && (cap == 0 || stats), "dsg_cc_stats_i32: cap=%d needs a stats buffer", cap);
  if (cap == 0) return DSG_OK;
  DSG_CHECK_ARG((reinterpret_cast<uintptr_t>(stats) & 7u) == 0, "dsg_cc_stats_i32: stats is not 8-byte aligned");
  const uint64_t label_bytes = (uint64_t)n * h * w * 4, stat_bytes = (uint64_t)n * cap * sizeof(dsg_cc_stat);
  DSG_CHECK_ARG(!dsg::overlap(stats, stat_bytes, labels, label_bytes), "dsg_cc_stats_i32: stats overlaps labels");
  DSG_CHECK_ARG(!dsg::overlap(stats, stat_bytes, counts, (uint64_t)n * 4), "dsg_cc_stats_i32: stats overlaps counts");
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(dsg::cc_stats_init_kernel, dim3(dsg::cdiv(cap, 256), n), dim3(256), 0, st, counts, cap, stats);
  DSG_LAUNCH_CHECK();
  const int tiles_x = dsg::cdiv(w, dsg::STAT_COLS), tiles_y = dsg::cdiv(h, dsg::STAT_ROWS);
  hipLaunchKernelGGL(dsg::cc_stats_kernel, dim3((unsigned)((int64_t)tiles_x * tiles_y), n), dim3(dsg::STAT_THREADS), 0, st,
                     labels, h, w, tiles_x, counts, cap, stats);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_cc_centers_i32(const dsg_cc_stat* stats, const int32_t* counts, int32_t n, int32_t cap, int32_t* coords,
                               void* stream) {
  DSG_CHECK_ARG(counts, "dsg_cc_centers_i32: NULL pointer");
  DSG_CHECK_ARG(n > 0 && n <= 65535, "dsg_cc_centers_i32: bad n=%d (1 .. 65535)", n);
  DSG_CHECK_ARG(cap >= 0 && (cap == 0 || (stats && coords)), "dsg_cc_centers_i32: cap=%d needs stats and coords", cap);
  if (cap == 0) return DSG_OK;
  const uint64_t stat_bytes = (uint64_t)n * cap * sizeof(dsg_cc_stat), coord_bytes = (uint64_t)n * cap * 8;
  DSG_CHECK_ARG(!dsg::overlap(coords, coord_bytes, stats, stat_bytes), "dsg_cc_centers_i32: coords overlaps stats");
  DSG_CHECK_ARG(!dsg::overlap(coords, coord_bytes, counts, (uint64_t)n * 4), "dsg_cc_centers_i32: coords overlaps counts");
  hipLaunchKernelGGL(dsg::cc_centers_kernel, dim3(dsg::cdiv(cap, 256), n), dim3(256), 0, static_cast<hipStream_t>(stream), stats,
                     counts, cap, coords);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}

DSG_API int dsg_merge_nodes_i32(int32_t* nodes, const int32_t* counts, int32_t n, int32_t cap, const int32_t* dense,
                                const int32_t* dense_counts, int32_t dense_cap, int64_t min_d2, int32_t* out_counts,
                                void* stream) {
  DSG_CHECK_ARG(counts && dense_counts && out_counts, "dsg_merge_nodes_i32: NULL pointer");
  DSG_CHECK_ARG(n > 0 && cap >= 0 && dense_cap >= 0 && (cap == 0 || nodes) && (dense_cap == 0 || dense),
                "dsg_merge_nodes_i32: bad arguments (n=%d cap=%d dense_cap=%d; a list with room needs a buffer)", n, cap, dense_cap);
  DSG_CHECK_ARG(min_d2 >= 0, "dsg_merge_nodes_i32: min_d2 is negative");
  const uint64_t node_bytes = (uint64_t)n * cap * 8, dense_bytes = (uint64_t)n * dense_cap * 8, cb = (uint64_t)n * 4;
  const void* ins[4] = {nodes, counts, dense, dense_counts};
  const uint64_t in_bytes[4] = {node_bytes, cb, dense_bytes, cb};
  for (int i = 0; i < 4; ++i)
    DSG_CHECK_ARG(!dsg::overlap(out_counts, cb, ins[i], in_bytes[i]), "dsg_merge_nodes_i32: out_counts overlaps argument %d", i);
  for (int i = 1; i < 4; ++i)
    DSG_CHECK_ARG(!dsg::overlap(nodes, node_bytes, ins[i], in_bytes[i]), "dsg_merge_nodes_i32: nodes overlaps argument %d", i);
  hipLaunchKernelGGL(dsg::merge_nodes_kernel, dim3(n), dim3(dsg::MERGE_NODES_THREADS), 0, static_cast<hipStream_t>(stream), nodes,
                     counts, cap, dense, dense_counts, dense_cap, (long long)min_d2, out_counts);
  DSG_LAUNCH_CHECK();
  return DSG_OK;
}
