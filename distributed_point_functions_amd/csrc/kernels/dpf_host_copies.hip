// dpf_host_copies.hip -- the host-only part of the C ABI (include/dpf_hip.h):
// device and page-locked allocation, copies between the device and pageable
// host memory (page-locked bounce buffers, reference-counted hipHostRegister,
// the helper-thread pipelined D2H), memset, and the stream / event / device
// wrappers.  No kernels: it needs dpf_runtime.h only.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <sys/mman.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <mutex>
#include <thread>
#include <vector>

#include "../../../include/dpf_hip.h"
#include "dpf_runtime.h"

using namespace dpf_rt;

namespace {
// Large copies between the device and pageable host memory: the runtime pins
// the user pages for each such copy, which measured ~28 ms per call for
// 4-128 MiB (tools/dpf_benchmark, BM_EvaluateRegularDpf at 2^22+ outputs)
// against ~0.3 ms for 16 MiB through page-locked memory.  They go through two
// page-locked 16 MiB bounce buffers instead, the DMA of one chunk overlapping
// the host copy of the other.
constexpr size_t kBounceMin = size_t{2} << 20;
constexpr size_t kBounceChunk = size_t{16} << 20;

// memcpy on up to 8 host threads for pieces of >= 2 MiB (the host side of a
// bounce runs at ~28 GB/s on 8 threads vs ~5 on one, page faults included).
void host_copy(void* dst, const void* src, size_t bytes) {
  const size_t piece = size_t{2} << 20;
  size_t t = bytes / piece;
  static const size_t hw = [] {
    const int v = hook_int("DPF_HOST_THREADS", 0);   // as host_util.h HostThreads()
    return v >= 1 ? static_cast<size_t>(v) : static_cast<size_t>(std::thread::hardware_concurrency());
  }();
  if (t > 8) t = 8;
  if (hw && t > hw) t = hw;
  if (t <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> pool;
  for (size_t i = 0; i < t; ++i) {
    const size_t lo = bytes * i / t, hi = bytes * (i + 1) / t;
    pool.emplace_back([=] { memcpy((char*)dst + lo, (const char*)src + lo, hi - lo); });
  }
  for (auto& th : pool) th.join();
}
std::mutex g_bounce_mu;
char* g_bounce[2] = {nullptr, nullptr};

bool page_locked(const void* p) {
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeDevice ||
         a.type == hipMemoryTypeManaged;
}

int bounce_buffers() {
  for (auto& b : g_bounce)
    if (!b) HIP_TRY(hipHostMalloc((void**)&b, kBounceChunk, hipHostMallocDefault));
  return kOk;
}

// Device memory to the host through the two bounce buffers, `chunk` bytes at a
// time: consume(ctx, buffer, offset, len) sees chunk i while the DMA of chunk
// i + 1 runs into the other buffer.  Takes g_bounce_mu.
int bounce_d2h_chunks(const void* src, size_t bytes, size_t chunk,
                      void (*consume)(void* ctx, const void* buf, size_t offset, size_t len),
                      void* ctx, hipStream_t s) {
  std::lock_guard<std::mutex> lock(g_bounce_mu);
  if (int rc = bounce_buffers()) return rc;
  const size_t n = (bytes + chunk - 1) / chunk;
  auto len = [&](size_t i) { return i + 1 < n ? chunk : bytes - i * chunk; };
  HIP_TRY(hipMemcpyAsync(g_bounce[0], src, len(0), hipMemcpyDeviceToHost, s));
  for (size_t i = 0; i < n; ++i) {
    HIP_TRY(hipStreamSynchronize(s));   // chunk i is in g_bounce[i & 1]
    if (i + 1 < n)
      HIP_TRY(hipMemcpyAsync(g_bounce[(i + 1) & 1], (const char*)src + (i + 1) * chunk, len(i + 1),
                             hipMemcpyDeviceToHost, s));
    // The next chunk's DMA into the other bounce buffer must have finished
    // before the buffers (and g_bounce_mu) are given up on any path out.
    try {
      consume(ctx, g_bounce[i & 1], i * chunk, len(i));
    } catch (...) {
      (void)hipStreamSynchronize(s);
      return fail(kInternal, "dpf_hip_memcpy_d2h_chunked: consume threw");
    }
  }
  return kOk;
}

int bounce_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  return bounce_d2h_chunks(
      src, bytes, kBounceChunk,
      [](void* d, const void* buf, size_t off, size_t len) { host_copy((char*)d + off, buf, len); },
      dst, (hipStream_t)stream);
}

// Large copies to or from pageable host memory: register the host range for
// the copy (16 ms for 8 GiB of mapped pages, tools/host_output_microbench.cc)
// and DMA straight into / out of it at the link rate (57 GB/s vs ~12 through
// the bounce buffers); the bounce path stays as the fallback when the
// registration is refused.
// Registering a fresh range (and unmapping it after) costs more than the
// page-locked staging below ~0.5 GiB (tools/fresh_output_microbench.cc,
// profiles/r14_fresh_output_microbench.jsonl): 32 MiB 4.5 vs 3.9 ms, 256 MiB
// 26.3 vs 25.9 ms; at 8 GiB the DMA straight into the range wins (42 vs ~28 GB/s).
constexpr size_t kRegisterMin = DPF_HIP_REGISTER_MIN_BYTES;
// The 512 MiB threshold prices the page faults of FRESH destinations.  A host
// range whose pages are already mapped -- every H2D source, and D2H
// destinations the caller has touched -- costs ~2 us/MiB to register (16 ms
// for 8 GiB, tools/host_output_microbench.cc) against a DMA at ~57 GB/s
// instead of ~12 GB/s through the bounce buffers, so those register from
// 32 MiB (the r13 threshold); profiles/r15_ab.txt (3), r15_mapped_register_ab.jsonl.
// DPF_HIP_REGISTER_MAPPED_MIB=<n> (read per call) overrides it: the A/B hook.
size_t register_min_mapped() {
  const long long m = hook_long("DPF_HIP_REGISTER_MAPPED_MIB", 0);
  return m > 0 ? static_cast<size_t>(m) << 20 : size_t{32} << 20;
}
// First, middle and last page of [p, p + bytes) resident (mincore): the
// range was touched before, so registering it maps no fresh pages.
bool pages_mapped(const void* p, size_t bytes) {
  const uintptr_t pg = 4096, lo = reinterpret_cast<uintptr_t>(p);
  for (uintptr_t a : {lo, lo + bytes / 2, lo + bytes - 1}) {
    unsigned char v = 0;
    if (mincore(reinterpret_cast<void*>(a & ~(pg - 1)), pg, &v) != 0 || !(v & 1)) return false;
  }
  return true;
}
constexpr size_t kStagedChunk = size_t{64} << 20;

// The library's own transient registrations, reference-counted: a second
// thread copying from or into a range another thread has registered for its
// copy shares that registration (page_locked() would report the range as
// page-locked and a plain async copy could outlive the first thread's
// hipHostUnregister); the last user unregisters.  A request that overlaps a
// registration without lying inside it takes the bounce path.
struct Registration {
  size_t bytes;
  int users;
};
std::mutex g_reg_mu;
std::map<uintptr_t, Registration> g_regs;   // base address -> registration
std::atomic<int> g_reg_count{0};            // g_regs.size(), readable without the lock

// Covers [p, p + bytes) with a library registration held by the caller (to be
// released with release_host(*base)): an existing one that contains the range,
// or -- for new ranges of >= kRegisterMin unless `reuse_only` -- a fresh one.
enum Acquire { kNotOurs, kAcquired, kOverlaps };
// kOverlaps: part of the range is in a registration of ours -- the copy must
// take the bounce path (HIP would take the partly registered range as
// page-locked).  kNotOurs: use the page-locked test / bounce path.
Acquire acquire_host(void* p, size_t bytes, bool reuse_only, uintptr_t* base,
                     size_t min_bytes = kRegisterMin) {
  const uintptr_t lo = reinterpret_cast<uintptr_t>(p), hi = lo + bytes;
  std::lock_guard<std::mutex> lock(g_reg_mu);
  auto it = g_regs.upper_bound(lo);
  if (it != g_regs.begin()) {
    auto prev = std::prev(it);
    if (prev->first + prev->second.bytes > lo) {          // overlaps the one below
      if (prev->first + prev->second.bytes >= hi) {        // contains the range
        ++prev->second.users;
        *base = prev->first;
        return kAcquired;
      }
      return kOverlaps;
    }
  }
  if (it != g_regs.end() && it->first < hi) return kOverlaps;  // overlaps the one above
  if (reuse_only || bytes < min_bytes) return kNotOurs;
  if (hipHostRegister(p, bytes, hipHostRegisterDefault) != hipSuccess) {
    (void)hipGetLastError();
    return kNotOurs;
  }
  g_regs[lo] = Registration{bytes, 1};
  g_reg_count.store(static_cast<int>(g_regs.size()));
  *base = lo;
  return kAcquired;
}

// True if [lo, hi) overlaps a registration of ours (g_reg_mu held).
bool overlaps_registration(uintptr_t lo, uintptr_t hi) {
  auto it = g_regs.upper_bound(lo);
  if (it != g_regs.begin()) {
    auto prev = std::prev(it);
    if (prev->first + prev->second.bytes > lo) return true;
  }
  return it != g_regs.end() && it->first < hi;
}

void release_host(uintptr_t base) {
  std::lock_guard<std::mutex> lock(g_reg_mu);
  auto it = g_regs.find(base);
  if (it == g_regs.end() || --it->second.users > 0) return;
  (void)hipHostUnregister(reinterpret_cast<void*>(base));
  g_regs.erase(it);
  g_reg_count.store(static_cast<int>(g_regs.size()));
}

// Copies chunk by chunk on `s`, calling before(ctx, end) ahead of each chunk's
// DMA (D2H: the destination chunk becomes valid while the previous chunk's
// DMA runs).  `h` lies in the registration acquired at `base`, released here.
int registered_copy(char* h, char* d, size_t bytes, bool to_host, void (*before)(void*, size_t),
                    void* ctx, hipStream_t s, uintptr_t base) {
  int rc = kOk;
  for (size_t off = 0; off < bytes && rc == kOk; off += kStagedChunk) {
    const size_t len = bytes - off < kStagedChunk ? bytes - off : kStagedChunk;
    if (before) before(ctx, off + len);
    const hipError_t e = to_host ? hipMemcpyAsync(h + off, d + off, len, hipMemcpyDeviceToHost, s)
                                 : hipMemcpyAsync(d + off, h + off, len, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (registered host memory)");
  }
  const hipError_t e = hipStreamSynchronize(s);
  if (rc == kOk && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
  release_host(base);
  return rc;
}

// Maps the pages of fresh host storage [p, p + bytes) by touching one byte per
// 4 KiB page on up to `threads` threads (a one-thread first touch of a fresh
// 8 GiB vector costs ~350 ms of page faults, tools/host_output_microbench.cc;
// registering unmapped pages would fault them in on one thread too).
void prefault(char* p, size_t bytes, int threads) {
  constexpr size_t kPage = 4096;
  const size_t pages = bytes / kPage + 1;
  size_t t = bytes >> 24;   // one thread per 16 MiB
  if (t > static_cast<size_t>(threads)) t = threads;
  auto touch = [p, bytes](size_t lo, size_t hi) {
    volatile char* v = p;
    for (size_t i = lo; i < hi; ++i)
      if (i * kPage < bytes) v[i * kPage] = 0;
  };
  if (t <= 1) {
    touch(0, pages);
    return;
  }
  std::vector<std::thread> pool;
  size_t done = 0;   // ranges [0, done) handed to threads
  try {
    for (; done < t; ++done) pool.emplace_back(touch, pages * done / t, pages * (done + 1) / t);
  } catch (...) {
    // No thread to spare: the rest on this one.
  }
  if (done < t) touch(pages * done / t, pages);
  for (auto& th : pool) th.join();
}

// A fresh destination of >= kRegisterMin is mapped and registered piece by
// piece behind the DMA (see piece_bytes below for the piece sizes).
// DPF_HIP_D2H_PIPELINE=0 (read per call) maps and registers the whole range
// before the first DMA instead (the r13 path): the A/B and test hook.
constexpr size_t kPipelineMax = size_t{16} << 30;   // above: a few large pieces
bool d2h_pipeline_on(size_t) { return !hook_is("DPF_HIP_D2H_PIPELINE", '0'); }
// DPF_HIP_D2H_REGISTER_PIECES=<n> (read per call): the pipelined copy acts as
// if the registration of its piece n (and every later one) were refused -- a
// test hook for the bounce fallback of the rest of the range.
long register_pieces_limit() { return (long)hook_long("DPF_HIP_D2H_REGISTER_PIECES", -1); }

// A fresh pageable destination of >= kRegisterMin (no registration of ours
// overlaps it): a helper thread maps (prefault, 8 threads) and registers it in
// pieces (256 MiB, or 1/32 of the range) while this thread initialises (before) and DMAs the pieces
// already registered, so the ~45 ms of mapping and registering 8 GiB runs
// under the DMA instead of ahead of it.  Piece boundaries are 2 MiB-aligned
// (no page in two registrations) and every DMA chunk lies in one piece.  A
// piece whose registration is refused, and everything after it, goes through
// the bounce buffers.
constexpr size_t kPiece = size_t{256} << 20;
constexpr int kNoHelperThread = -1000;   // pipelined_d2h could not start its helper
// Up to kPipelineMax: ~32 pieces (256 MiB up to 8 GiB; 8 GiB copies 164-171
// ms pipelined vs 199-209 ms registered whole).  Above it, 8 GiB pieces: a
// 32 GiB copy (config 3's 2^31 uint128) in 33 or 129 pieces ran its DMA at
// ~13 GB/s in 1 of 4 calls (r14) and 3 of 6 (r15), in 5 pieces never in 6
// calls (3 pieces: never in 6), 682-758 ms per copy against 801-938 ms
// registered whole first (profiles/r15_ab.txt part 12).  A/B hooks (read per
// call): DPF_HIP_D2H_PIECE_MIB (a multiple of 64) and
// DPF_HIP_D2H_PREFAULT_THREADS (default 8).

size_t piece_bytes(size_t bytes) {
  const long long m = hook_long("DPF_HIP_D2H_PIECE_MIB", 0);
  if (m >= 64 && m % 64 == 0) return static_cast<size_t>(m) << 20;
  const size_t step = size_t{64} << 20;
  if (bytes > kPipelineMax) return size_t{8} << 30;
  const size_t want = (bytes / 32 + step - 1) / step * step;
  return want > kPiece ? want : kPiece;
}
int prefault_threads() {
  const long long t = hook_long("DPF_HIP_D2H_PREFAULT_THREADS", 0);
  return t >= 1 && t <= 64 ? static_cast<int>(t) : 8;
}

// With parts (nparts > 0) the DMAs run on `s` = a copy stream of their own:
// [0, ends[j]) of `d` is ready once events[j] (recorded on the producing
// stream) has completed, and each chunk's DMA waits on the device for the
// first part that covers it, so the copy of part j overlaps the work that
// produces the later parts.
int pipelined_d2h(char* h, const char* d, size_t bytes, void (*before)(void*, size_t), void* ctx,
                  hipStream_t s, int nparts = 0, void* const* events = nullptr,
                  const size_t* ends = nullptr) {
  const uintptr_t h0 = reinterpret_cast<uintptr_t>(h), h1 = h0 + bytes;
  const size_t piece = piece_bytes(bytes);
  const int pf_threads = prefault_threads();
  std::vector<uintptr_t> cut{h0};   // piece i = [cut[i], cut[i + 1])
  for (uintptr_t c = (h0 + piece) & ~((uintptr_t{2} << 20) - 1); c < h1; c += piece)
    if (c > cut.back()) cut.push_back(c);
  cut.push_back(h1);
  const size_t n = cut.size() - 1;
  std::vector<int> state(n, 0);   // 0 pending, 1 registered (in g_regs), -1 refused
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<bool> stop{false};
  int device = 0;
  (void)hipGetDevice(&device);
  const long limit = register_pieces_limit();
  // DPF_HIP_D2H_TRACE=1: per-call seconds spent mapping, registering and
  // waiting for the helper thread, on stderr (a diagnostic).
  const bool trace = hook_set("DPF_HIP_D2H_TRACE");
  using clk = std::chrono::steady_clock;
  double t_fault = 0, t_reg = 0, t_wait = 0, t_before = 0;
  const auto t_start = clk::now();
  std::thread worker;
  auto helper = [&] {
    (void)hipSetDevice(device);
    for (size_t i = 0; i < n && !stop.load(); ++i) {
      char* p = reinterpret_cast<char*>(cut[i]);
      const size_t len = cut[i + 1] - cut[i];
      const auto a = clk::now();
      prefault(p, len, pf_threads);
      const auto b = clk::now();
      int st = -1;
      if (limit >= 0 && static_cast<long>(i) >= limit) {
        // test hook: refused
      } else {
        // Under g_reg_mu from the overlap check to the insert: another thread
        // may have registered part of this piece since acquire_host said
        // kNotOurs.  An overlapping piece is refused (the bounce path).
        std::lock_guard<std::mutex> lock(g_reg_mu);
        if (!overlaps_registration(cut[i], cut[i + 1])) {
          if (hipHostRegister(p, len, hipHostRegisterDefault) == hipSuccess) {
            g_regs[cut[i]] = Registration{len, 1};
            g_reg_count.store(static_cast<int>(g_regs.size()));
            st = 1;
          } else {
            (void)hipGetLastError();
          }
        }
      }
      t_fault += std::chrono::duration<double>(b - a).count();
      t_reg += std::chrono::duration<double>(clk::now() - b).count();
      {
        std::lock_guard<std::mutex> lock(mu);
        state[i] = st;
      }
      cv.notify_all();
      if (st < 0) break;
    }
  };
  try {
    worker = std::thread(helper);
  } catch (...) {
    return kNoHelperThread;   // nothing done yet: the caller copies another way
  }
  int rc = kOk;
  int waited = -1;   // parts whose event `s` already waits for: [0, waited]
  auto wait_parts = [&](size_t end) {
    int j = waited + 1;
    while (j < nparts - 1 && ends[j] < end) ++j;
    if (j >= nparts || j <= waited) return;
    const hipError_t e = hipStreamWaitEvent(s, (hipEvent_t)events[j], 0);
    if (e != hipSuccess) rc = hip_fail(e, "hipStreamWaitEvent");
    waited = j;
  };
  size_t i = 0;
  for (; i < n && rc == kOk; ++i) {
    int st;
    {
      const auto w = clk::now();
      std::unique_lock<std::mutex> lock(mu);
      cv.wait(lock, [&] { return state[i] != 0; });
      st = state[i];
      t_wait += std::chrono::duration<double>(clk::now() - w).count();
    }
    if (st < 0) break;
    for (uintptr_t off = cut[i]; off < cut[i + 1] && rc == kOk; off += kStagedChunk) {
      const size_t len = cut[i + 1] - off < kStagedChunk ? cut[i + 1] - off : kStagedChunk;
      wait_parts(off + len - h0);
      if (rc != kOk) break;
      if (before) {
        // The helper thread must be joined on every path out of here.
        try {
          const auto bt = clk::now();
          before(ctx, off + len - h0);
          t_before += std::chrono::duration<double>(clk::now() - bt).count();
        } catch (...) {
          rc = fail(kInternal, "dpf_hip_memcpy_d2h_staged: before_chunk threw");
          break;
        }
      }
      const hipError_t e = hipMemcpyAsync(reinterpret_cast<char*>(off), d + (off - h0), len,
                                          hipMemcpyDeviceToHost, s);
      if (e != hipSuccess) rc = hip_fail(e, "hipMemcpyAsync (registered host memory)");
    }
  }
  stop.store(true);
  worker.join();
  if (rc == kOk && i < n) {
    // Registration refused from piece i on: the rest through the bounce buffers.
    const size_t off = cut[i] - h0;
    prefault(h + off, bytes - off, 8);
    try {
      if (before) before(ctx, bytes);
    } catch (...) {
      rc = fail(kInternal, "dpf_hip_memcpy_d2h_staged: before_chunk threw");
    }
    if (rc == kOk) wait_parts(bytes);
    if (rc == kOk) rc = bounce_d2h(h + off, d + off, bytes - off, s);
  }
  const auto t_issue = clk::now();
  const hipError_t e = hipStreamSynchronize(s);
  if (rc == kOk && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize");
  const auto t_sync = clk::now();
  for (size_t j = 0; j < n; ++j)
    if (state[j] > 0) release_host(cut[j]);
  if (trace)
    fprintf(stderr, "[pipelined_d2h] %zu MiB in %zu pieces: total %.1f ms, map %.1f ms, register "
            "%.1f ms (helper), wait %.1f ms, before_chunk %.1f ms, issue %.1f ms, final sync "
            "%.1f ms, unregister %.1f ms\n", bytes >> 20, n,
            1e3 * std::chrono::duration<double>(clk::now() - t_start).count(), 1e3 * t_fault,
            1e3 * t_reg, 1e3 * t_wait, 1e3 * t_before,
            1e3 * std::chrono::duration<double>(t_issue - t_start).count(),
            1e3 * std::chrono::duration<double>(t_sync - t_issue).count(),
            1e3 * std::chrono::duration<double>(clk::now() - t_sync).count());
  return rc;
}

int bounce_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  std::lock_guard<std::mutex> lock(g_bounce_mu);
  if (int rc = bounce_buffers()) return rc;
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (bytes + kBounceChunk - 1) / kBounceChunk;
  for (size_t i = 0; i < n; ++i) {
    const size_t l = i + 1 < n ? kBounceChunk : bytes - i * kBounceChunk;
    if (i >= 2) HIP_TRY(hipStreamSynchronize(s));   // chunk i - 2 has left g_bounce[i & 1]
    host_copy(g_bounce[i & 1], (const char*)src + i * kBounceChunk, l);
    HIP_TRY(hipMemcpyAsync((char*)dst + i * kBounceChunk, g_bounce[i & 1], l,
                           hipMemcpyHostToDevice, s));
  }
  HIP_TRY(hipStreamSynchronize(s));
  return kOk;
}
}  // namespace

extern "C" {

int dpf_hip_device_count(int* count) {
  HIP_TRY(hipGetDeviceCount(count));
  return kOk;
}
int dpf_hip_set_device(int device) {
  HIP_TRY(hipSetDevice(device));
  return kOk;
}
int dpf_hip_alloc(void** ptr, size_t bytes) {
  if (!ptr) return fail(kInvalidArgument, "ptr is NULL");
  *ptr = nullptr;
  if (bytes == 0) bytes = 1;
  const hipError_t e = hipMalloc(ptr, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();  // an allocation failure must not fail the next launch check
    *ptr = nullptr;
  }
  HIP_TRY(e);
  return kOk;
}
int dpf_hip_mem_info(size_t* free_bytes, size_t* total_bytes) {
  if (!free_bytes || !total_bytes) return fail(kInvalidArgument, "NULL pointer");
  HIP_TRY(hipMemGetInfo(free_bytes, total_bytes));
  return kOk;
}
int dpf_hip_free(void* ptr) {
  if (ptr) HIP_TRY(hipFree(ptr));
  return kOk;
}
int dpf_hip_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (!bytes) return kOk;
  uintptr_t base = 0;
  if (bytes >= kBounceMin || g_reg_count.load() > 0) {
    // Inside a registration of ours (another thread's copy), or large and new.
    const Acquire a = acquire_host(const_cast<void*>(src), bytes,
                                   bytes < kBounceMin || page_locked(src), &base,
                                   register_min_mapped());
    if (a == kAcquired)
      return registered_copy((char*)const_cast<void*>(src), (char*)dst, bytes, false, nullptr,
                             nullptr, (hipStream_t)stream, base);
    if (a == kOverlaps || (bytes >= kBounceMin && !page_locked(src)))
      return bounce_h2d(dst, src, bytes, stream);
  }
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return kOk;
}
int dpf_hip_host_alloc(void** ptr, size_t bytes) {
  if (!ptr) return fail(kInvalidArgument, "ptr is NULL");
  *ptr = nullptr;
  if (bytes == 0) bytes = 1;
  HIP_TRY(hipHostMalloc(ptr, bytes, hipHostMallocDefault));
  return kOk;
}
int dpf_hip_host_free(void* ptr) {
  if (ptr) HIP_TRY(hipHostFree(ptr));
  return kOk;
}
int dpf_hip_memcpy_h2d_async(void* dst, const void* src, size_t bytes, void* stream) {
  if (!bytes) return kOk;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  return kOk;
}
int dpf_hip_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  if (!bytes) return kOk;
  uintptr_t base = 0;
  if (bytes >= kBounceMin || g_reg_count.load() > 0) {
    const bool reuse_only = bytes < kBounceMin || page_locked(dst);
    const Acquire a =
        acquire_host(dst, bytes, reuse_only, &base,
                     !reuse_only && pages_mapped(dst, bytes) ? register_min_mapped() : kRegisterMin);
    if (a == kAcquired)
      return registered_copy((char*)dst, (char*)const_cast<void*>(src), bytes, true, nullptr,
                             nullptr, (hipStream_t)stream, base);
    if (a == kOverlaps || (bytes >= kBounceMin && !page_locked(dst)))
      return bounce_d2h(dst, src, bytes, stream);
  }
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return kOk;
}
int dpf_hip_memcpy_d2h_strided(void* dst, const void* src, size_t elem_bytes,
                               size_t src_stride_bytes, int64_t count, void* stream) {
  if (count < 0 || src_stride_bytes < elem_bytes) return fail(kInvalidArgument, "bad sizes");
  if (count == 0 || elem_bytes == 0) return kOk;
  if (!dst || !src) return fail(kInvalidArgument, "NULL pointer");
  HIP_TRY(hipMemcpy2DAsync(dst, elem_bytes, src, src_stride_bytes, elem_bytes, (size_t)count,
                           hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return kOk;
}
int dpf_hip_memcpy_d2h_staged(void* dst, const void* src, size_t bytes,
                              void (*before_chunk)(void* ctx, size_t bytes_ready), void* ctx,
                              void* stream) {
  return dpf_hip_memcpy_d2h_staged_after(dst, src, bytes, before_chunk, ctx, 0, nullptr, nullptr,
                                         stream);
}
int dpf_hip_memcpy_d2h_staged_after(void* dst, const void* src, size_t bytes,
                                    void (*before_chunk)(void* ctx, size_t bytes_ready), void* ctx,
                                    int num_parts, void* const* part_events,
                                    const size_t* part_end_bytes, void* stream) {
  if (num_parts < 0 || (num_parts > 0 && (!part_events || !part_end_bytes)))
    return fail(kInvalidArgument, "dpf_hip_memcpy_d2h_staged_after: bad parts");
  for (int j = 0; j < num_parts; ++j)
    if (!part_events[j] || (j > 0 && part_end_bytes[j] < part_end_bytes[j - 1]) ||
        (j == num_parts - 1 && part_end_bytes[j] < bytes))
      return fail(kInvalidArgument, "dpf_hip_memcpy_d2h_staged_after: bad parts");
  // Every path but the pipelined one copies on `stream`, after all its parts.
  if (!before_chunk) return dpf_hip_memcpy_d2h(dst, src, bytes, stream);
  uintptr_t base = 0;
  if (bytes >= kRegisterMin) {
    const bool locked = page_locked(dst);
    // An existing registration of ours that contains the range is shared;
    // a fresh pageable range is mapped and registered piece by piece.
    const Acquire a = acquire_host(dst, bytes, true, &base);
    if (a == kAcquired)
      return registered_copy((char*)dst, (char*)const_cast<void*>(src), bytes, true, before_chunk,
                             ctx, (hipStream_t)stream, base);
    if (a == kNotOurs && !locked) {
      if (d2h_pipeline_on(bytes)) {
        int rc;
        if (num_parts == 0) {
          rc = pipelined_d2h((char*)dst, (const char*)src, bytes, before_chunk, ctx,
                             (hipStream_t)stream);
        } else {
          hipStream_t copy;
          HIP_TRY(hipStreamCreateWithFlags(&copy, hipStreamNonBlocking));
          rc = pipelined_d2h((char*)dst, (const char*)src, bytes, before_chunk, ctx, copy,
                             num_parts, part_events, part_end_bytes);
          (void)hipStreamDestroy(copy);
        }
        if (rc != kNoHelperThread) return rc;
        // No helper thread: map and register the whole range first.
      }
      using clk = std::chrono::steady_clock;
      const auto t0 = clk::now();
      prefault((char*)dst, bytes, 16);
      const auto t1 = clk::now();
      if (acquire_host(dst, bytes, false, &base) == kAcquired) {
        const auto t2 = clk::now();
        const int rc = registered_copy((char*)dst, (char*)const_cast<void*>(src), bytes, true,
                                       before_chunk, ctx, (hipStream_t)stream, base);
        if (hook_set("DPF_HIP_D2H_TRACE"))
          fprintf(stderr, "[whole_d2h] %zu MiB: total %.1f ms, map %.1f ms, register %.1f ms, "
                  "copy+unregister %.1f ms\n", bytes >> 20,
                  1e3 * std::chrono::duration<double>(clk::now() - t0).count(),
                  1e3 * std::chrono::duration<double>(t1 - t0).count(),
                  1e3 * std::chrono::duration<double>(t2 - t1).count(),
                  1e3 * std::chrono::duration<double>(clk::now() - t2).count());
        return rc;
      }
    }
  }
  before_chunk(ctx, bytes);
  return dpf_hip_memcpy_d2h(dst, src, bytes, stream);
}
int dpf_hip_memcpy_d2h_chunked(const void* src, size_t bytes, size_t align,
                               void (*consume)(void* ctx, const void* chunk, size_t offset,
                                               size_t len),
                               void* ctx, void* stream) {
  if (!bytes) return kOk;
  if (!src || !consume || align == 0 || align > kBounceChunk)
    return fail(kInvalidArgument, "dpf_hip_memcpy_d2h_chunked: bad arguments");
  return bounce_d2h_chunks(src, bytes, kBounceChunk / align * align, consume, ctx,
                           (hipStream_t)stream);
}
int dpf_hip_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (!bytes) return kOk;
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return kOk;
}
int dpf_hip_memset(void* dst, int value, size_t bytes, void* stream) {
  if (!bytes) return kOk;
  HIP_TRY(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
  return kOk;
}
int dpf_hip_stream_sync(void* stream) {
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  return kOk;
}
int dpf_hip_event_sync(void* event) {
  HIP_TRY(hipEventSynchronize((hipEvent_t)event));
  return kOk;
}
int dpf_hip_stream_wait_event(void* stream, void* event) {
  HIP_TRY(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
  return kOk;
}
int dpf_hip_event_create(void** ev) {
  HIP_TRY(hipEventCreate((hipEvent_t*)ev));
  return kOk;
}
int dpf_hip_event_destroy(void* ev) {
  HIP_TRY(hipEventDestroy((hipEvent_t)ev));
  return kOk;
}
int dpf_hip_event_record(void* ev, void* stream) {
  HIP_TRY(hipEventRecord((hipEvent_t)ev, (hipStream_t)stream));
  return kOk;
}
int dpf_hip_event_elapsed_ms(void* start, void* stop, float* ms) {
  HIP_TRY(hipEventSynchronize((hipEvent_t)stop));
  HIP_TRY(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return kOk;
}

}  // extern "C"
