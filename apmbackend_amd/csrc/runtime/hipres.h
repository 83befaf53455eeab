// apm::HipRes -- the one owner of a runtime object's GPU resources: device blocks, pinned host
// blocks, events and streams.  Engine, DeviceJoin and the host collective each hold one; nothing
// else under runtime/ calls the HIP allocation / creation / destruction entry points.
//
// Members that point into the owner's resources are plain pointers (or the small handles below):
// whoever holds the owner quiesces its streams and threads, then calls release_all() once.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <mutex>
#include <unordered_map>
#include <vector>

namespace apm {

// Process-wide live counts over every HipRes (bindings: _apm_native.live_resources()).
struct LiveResources {
  std::atomic<int64_t> device_blocks{0}, device_bytes{0}, pinned_blocks{0}, pinned_bytes{0}, events{0}, streams{0};
};
LiveResources& live_resources();

// A pinned block with its device alias (zero-copy: kernels write `d`, the host reads `h`).
template <class T>
struct Mapped {
  T* h = nullptr;
  T* d = nullptr;
  operator T*() const { return h; }
};

// A growable pinned buffer: pointer + capacity in elements of T (HipRes::reserve), with the
// device alias when it was asked for.
template <class T>
struct PinnedBuf {
  T* p = nullptr;
  T* d = nullptr;
  size_t cap = 0;
  operator T*() const { return p; }
};

class HipRes {
 public:
  HipRes() = default;
  HipRes(const HipRes&) = delete;
  HipRes& operator=(const HipRes&) = delete;
  ~HipRes() { release_all(); }

  // ---- device blocks (sizes round up to 256 bytes, dmalloc_raw aside; thread-safe)
  void* dmalloc(size_t bytes);                         // zeroed; syncs the null stream only
  void* dmalloc_on(hipStream_t s, size_t bytes);       // zeroed in order on `s`, no sync
  void* dmalloc_try(size_t bytes);                     // nullptr when HBM is short; not zeroed
  void* dmalloc_raw(size_t bytes);                     // exact size, not zeroed, no sync; failure is fatal
  void dfree(void* p);                                 // nullptr is fine
  void* regrow(void* old, size_t& cap, size_t need, hipStream_t s);
  size_t device_bytes() const { return device_bytes_.load(std::memory_order_relaxed); }

  // ---- pinned blocks
  void* pinned(size_t bytes, void** dev_alias = nullptr);
  template <class T>
  void pin(T*& h, size_t bytes) { h = (T*)pinned(bytes); }
  template <class T>
  void pin(Mapped<T>& m, size_t bytes) { m.h = (T*)pinned(bytes, (void**)&m.d); }
  // Grows `b` to `new_cap` elements when it holds fewer than `need` (the old block is freed, its
  // contents are not kept).  The caller picks new_cap: each site has its own headroom rule.
  template <class T>
  bool reserve(PinnedBuf<T>& b, size_t need, size_t new_cap, bool alias = false) {
    if (need <= b.cap) return false;
    pfree(b.p);
    b.d = nullptr;
    b.p = (T*)pinned(new_cap * sizeof(T), alias ? (void**)&b.d : nullptr);
    b.cap = new_cap;
    return true;
  }
  void pfree(void* p);   // nullptr is fine
  // Drops a pinned block from the books without freeing it (a sink still reads it: ~Engine).
  void forget(void* p);
  static void* device_alias(const void* pinned_host);

  // ---- events (hipEventDisableTiming) and streams (created by the caller, destroyed here)
  hipEvent_t new_event();
  hipStream_t adopt(hipStream_t s);

  // Events, then pinned blocks, then device blocks, then streams.  Idempotent.
  void release_all();

 private:
  void* track(void* p, size_t bytes);
  mutable std::mutex mu_;
  std::unordered_map<void*, size_t> dev_, pin_;
  std::vector<hipEvent_t> events_;
  std::vector<hipStream_t> streams_;
  std::atomic<size_t> device_bytes_{0};
};

// A pinned block for one scope (the checkpoint bounce buffers).
struct ScopedPinned {
  HipRes& res;
  void* p;
  ScopedPinned(HipRes& r, size_t bytes) : res(r), p(r.pinned(bytes)) {}
  ~ScopedPinned() { res.pfree(p); }
  ScopedPinned(const ScopedPinned&) = delete;
  ScopedPinned& operator=(const ScopedPinned&) = delete;
};

}  // namespace apm
