// Red-zone device allocator for the bounds tests (tests/redzone_child.py, tests/test_gpu_redzones.py).
//
// Loaded into torch through torch.cuda.memory.CUDAPluggableAllocator: every torch allocation becomes its own hipMalloc,
//
//   [ head zone: G bytes ][ user region, 256-byte aligned, `size` bytes ][ slack: round_up(size, 256) - size ][ tail zone: G bytes ]
//
// and the whole span is filled with the current fill word before the pointer is handed out, so the user region starts as
// that word too (a read of memory no kernel wrote shows up as a result that depends on the word).  The zones (the slack is
// part of the tail) are compared with the word at free and on rz_check_live(); a mismatch is recorded, never thrown.
// Host code only: the fills are hipMemsetD32 / hipMemcpy, the checks run on the host.
//
//   hipcc --offload-arch=gfx950 -shared -fPIC -O2 -o libredzone.so redzone_alloc.cpp
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

namespace {

constexpr size_t kAlign = 256;
constexpr size_t kGuard = size_t(1) << 20;

struct Alloc {
  char* base;
  size_t size;
  uint64_t serial;
  uint32_t word;       // what the zones hold
  bool bad[2];         // head / tail already reported
};

struct Violation {
  uint64_t serial;
  size_t size;
  int side;            // 0 head, 1 tail
  size_t offset;       // first bad byte, from the zone's start (the tail zone starts right after the user's `size` bytes)
  size_t nbad;
  std::vector<uint8_t> bytes;   // up to 32 bytes from `offset` on
};

std::mutex g_mu;
std::map<uintptr_t, Alloc> g_live;
std::vector<Violation> g_viol;
uint64_t g_serial = 0;
uint32_t g_word = 0xFFFFFFFFu;
hipError_t g_last_err = hipSuccess;

size_t round_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

void layout_of(size_t size, size_t guard, size_t* out) {
  out[0] = guard;                                    // user offset (= head zone length)
  out[1] = round_up(size, kAlign) - size;            // tail slack
  out[2] = guard + size;                             // tail zone offset (slack first)
  out[3] = out[1] + guard;                           // tail zone length
  out[4] = 2 * guard + round_up(size, kAlign);       // bytes allocated
}

uint8_t want_byte(uint32_t word, size_t abs_off) { return uint8_t(word >> (8 * (abs_off & 3))); }

// compares bytes [off, off + len) of the allocation (offsets from base) with the word; records a violation on mismatch
int check_span(Alloc& a, int side, size_t off, size_t len, size_t zone_start) {
  if (a.bad[side] || len == 0) return 0;
  std::vector<uint8_t> host(len);
  hipError_t e = hipMemcpy(host.data(), a.base + off, len, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    g_last_err = e;
    return 0;
  }
  size_t first = len, nbad = 0;
  for (size_t i = 0; i < len; ++i) {
    if (host[i] != want_byte(a.word, off + i)) {
      if (first == len) first = i;
      ++nbad;
    }
  }
  if (!nbad) return 0;
  Violation v;
  v.serial = a.serial;
  v.size = a.size;
  v.side = side;
  v.offset = off + first - zone_start;
  v.nbad = nbad;
  v.bytes.assign(host.begin() + first, host.begin() + std::min(len, first + 32));
  g_viol.push_back(std::move(v));
  a.bad[side] = true;
  return 1;
}

int check_alloc(Alloc& a) {
  size_t lay[5];
  layout_of(a.size, kGuard, lay);
  return check_span(a, 0, 0, lay[0], 0) + check_span(a, 1, lay[2], lay[3], lay[2]);
}

}  // namespace

extern "C" {

// out[5] = {user offset, slack, tail zone offset, tail zone length, total bytes} of an allocation of `size` bytes with
// `guard`-byte zones (guard = 0: the built-in 1 MiB).  Pure arithmetic: usable without a GPU.
__attribute__((visibility("default"))) void rz_layout(size_t size, size_t guard, size_t* out) {
  layout_of(size, guard ? guard : kGuard, out);
}

__attribute__((visibility("default"))) void* rz_alloc(size_t size, int device, hipStream_t) {
  std::lock_guard<std::mutex> lk(g_mu);
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != device) (void)hipSetDevice(device);
  size_t lay[5];
  layout_of(size, kGuard, lay);
  void* base = nullptr;
  hipError_t e = hipMalloc(&base, lay[4]);
  if (e == hipSuccess) e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(base), int(g_word), lay[4] / 4);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (prev != device && prev >= 0) (void)hipSetDevice(prev);
  if (e != hipSuccess) {
    g_last_err = e;
    if (base) (void)hipFree(base);
    return nullptr;
  }
  char* user = static_cast<char*>(base) + lay[0];
  g_live[reinterpret_cast<uintptr_t>(user)] = Alloc{static_cast<char*>(base), size, ++g_serial, g_word, {false, false}};
  return user;
}

__attribute__((visibility("default"))) void rz_free(void* ptr, size_t, int device, hipStream_t) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_live.find(reinterpret_cast<uintptr_t>(ptr));
  if (it == g_live.end()) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (prev != device) (void)hipSetDevice(device);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) g_last_err = e;
  check_alloc(it->second);
  (void)hipFree(it->second.base);
  g_live.erase(it);
  if (prev != device && prev >= 0) (void)hipSetDevice(prev);
}

__attribute__((visibility("default"))) void rz_set_word(uint32_t word) {
  std::lock_guard<std::mutex> lk(g_mu);
  g_word = word;
}

// checks every live allocation now; returns the number of violations found by this call
__attribute__((visibility("default"))) int rz_check_live() {
  std::lock_guard<std::mutex> lk(g_mu);
  hipError_t e = hipDeviceSynchronize();
  if (e != hipSuccess) g_last_err = e;
  int n = 0;
  for (auto& kv : g_live) n += check_alloc(kv.second);
  return n;
}

__attribute__((visibility("default"))) int64_t rz_violation_count() {
  std::lock_guard<std::mutex> lk(g_mu);
  return int64_t(g_viol.size());
}

// the records as a JSON list; returns the length the whole text needs (write it again with a larger buffer if >= cap)
__attribute__((visibility("default"))) int64_t rz_violations(char* buf, int64_t cap) {
  std::lock_guard<std::mutex> lk(g_mu);
  std::string s = "[";
  char tmp[160];
  for (size_t i = 0; i < g_viol.size(); ++i) {
    const Violation& v = g_viol[i];
    snprintf(tmp, sizeof tmp, "%s{\"serial\": %llu, \"size\": %llu, \"side\": \"%s\", \"offset\": %llu, \"nbad\": %llu, \"bytes\": \"",
             i ? ", " : "", (unsigned long long)v.serial, (unsigned long long)v.size, v.side ? "tail" : "head",
             (unsigned long long)v.offset, (unsigned long long)v.nbad);
    s += tmp;
    for (uint8_t b : v.bytes) {
      snprintf(tmp, sizeof tmp, "%02x", b);
      s += tmp;
    }
    s += "\"}";
  }
  s += "]";
  if (buf && cap > 0) {
    size_t n = std::min(s.size(), size_t(cap - 1));
    memcpy(buf, s.data(), n);
    buf[n] = 0;
  }
  return int64_t(s.size()) + 1;
}

__attribute__((visibility("default"))) uint64_t rz_serial() {
  std::lock_guard<std::mutex> lk(g_mu);
  return g_serial;
}

// serial of the live allocation whose user region starts at ptr (0: not one of ours)
__attribute__((visibility("default"))) uint64_t rz_serial_of(void* ptr) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_live.find(reinterpret_cast<uintptr_t>(ptr));
  return it == g_live.end() ? 0 : it->second.serial;
}

// overwrites the zones (and slack) of the allocation at ptr with `word`, which its checks then expect; 0 on success
__attribute__((visibility("default"))) int rz_fill_zones(void* ptr, uint32_t word) {
  std::lock_guard<std::mutex> lk(g_mu);
  auto it = g_live.find(reinterpret_cast<uintptr_t>(ptr));
  if (it == g_live.end()) return -1;
  Alloc& a = it->second;
  size_t lay[5];
  layout_of(a.size, kGuard, lay);
  hipError_t e = hipDeviceSynchronize();
  std::vector<uint8_t> host(lay[3]);
  for (size_t i = 0; i < host.size(); ++i) host[i] = want_byte(word, lay[2] + i);
  if (e == hipSuccess) e = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(a.base), int(word), lay[0] / 4);
  if (e == hipSuccess) e = hipMemcpy(a.base + lay[2], host.data(), host.size(), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e != hipSuccess) {
    g_last_err = e;
    return -2;
  }
  a.word = word;
  return 0;
}

// last HIP error the allocator met (0: none), cleared by the call
__attribute__((visibility("default"))) int rz_last_error() {
  std::lock_guard<std::mutex> lk(g_mu);
  int e = int(g_last_err);
  g_last_err = hipSuccess;
  return e;
}

}  // extern "C"
