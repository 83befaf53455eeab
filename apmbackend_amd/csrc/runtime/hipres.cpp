#include "hipres.h"

#include <algorithm>

#include "../kernels/common.h"

namespace apm {

LiveResources& live_resources() {
  static LiveResources r;
  return r;
}

static size_t round256(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

void* HipRes::track(void* p, size_t bytes) {
  std::lock_guard<std::mutex> g(mu_);  // the stats thread and the rollover lane allocate
  dev_[p] = bytes;
  device_bytes_ += bytes;
  live_resources().device_blocks += 1;
  live_resources().device_bytes += (int64_t)bytes;
  return p;
}

void* HipRes::dmalloc(size_t bytes) {
  void* p = nullptr;
  bytes = round256(bytes);
  HIP_OK(hipMalloc(&p, bytes));
  HIP_OK(hipMemset(p, 0, bytes));
  // hipMemset runs on the null stream, which does not order against the engine's non-blocking
  // streams: without this wait, a buffer regrown mid-run could be zeroed *after* the first copy
  // into it on the stats stream (seen: K12 names table read back as zeros after a regrow).  The
  // null stream only, not the device: a device-wide sync would also wait for the collective stream
  // (a lock-step all-reduce waiting for a peer rank).
  HIP_OK(hipStreamSynchronize(nullptr));
  return track(p, bytes);
}

void* HipRes::dmalloc_on(hipStream_t s, size_t bytes) {
  void* p = nullptr;
  bytes = round256(bytes);
  HIP_OK(hipMalloc(&p, bytes));
  HIP_OK(hipMemsetAsync(p, 0, bytes, s));
  return track(p, bytes);
}

// Optional scratch (checkpoint packing and staging): nullptr instead of an abort when HBM is
// short, no zeroing and no sync; counted and freed like every other block.
void* HipRes::dmalloc_try(size_t bytes) {
  void* p = nullptr;
  bytes = round256(bytes);
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  return track(p, bytes);
}

// The blocks that were plain hipMalloc calls (text staging, name tables, checkpoint temporaries):
// the caller's exact size, no rounding.
void* HipRes::dmalloc_raw(size_t bytes) {
  void* p = nullptr;
  HIP_OK(hipMalloc(&p, bytes));
  return track(p, bytes);
}

// Frees a device block and forgets it (release_all frees what is still listed).
void HipRes::dfree(void* p) {
  if (!p) return;
  HIP_OK(hipFree(p));
  std::lock_guard<std::mutex> g(mu_);
  auto it = dev_.find(p);
  if (it == dev_.end()) return;
  device_bytes_ -= it->second;
  live_resources().device_blocks -= 1;
  live_resources().device_bytes -= (int64_t)it->second;
  dev_.erase(it);
}

void* HipRes::regrow(void* old, size_t& cap, size_t need, hipStream_t s) {
  if (need <= cap && old) return old;
  // 2x headroom: a regrow syncs the stream and hipFree waits for the device (a few ms of one
  // batch), so the per-batch buffers must stop growing during the warm-up
  const size_t nc = std::max<size_t>(2 * need, 4 << 20);
  // The old buffer is retired, not freed: kernels still in flight on any stream may read it, and
  // hipFree would wait for the whole device (the collective stream included).  Retired buffers
  // stay listed (and counted) until release_all; with 2x growth they add up to less than the
  // live buffer.
  cap = nc;
  // zeroed in order on `s` (the stats stream); the sync orders it for the other streams' later
  // work without waiting for them (dmalloc's null-stream sync is for construction time)
  void* p = dmalloc_on(s, nc);
  HIP_OK(hipStreamSynchronize(s));
  return p;
}

void* HipRes::pinned(size_t bytes, void** dev_alias) {
  void* p = nullptr;
  HIP_OK(hipHostMalloc(&p, bytes, hipHostMallocDefault));
  if (dev_alias) HIP_OK(hipHostGetDevicePointer(dev_alias, p, 0));
  std::lock_guard<std::mutex> g(mu_);
  pin_[p] = bytes;
  live_resources().pinned_blocks += 1;
  live_resources().pinned_bytes += (int64_t)bytes;
  return p;
}

void HipRes::forget(void* p) {
  std::lock_guard<std::mutex> g(mu_);
  auto it = pin_.find(p);
  if (it == pin_.end()) return;
  live_resources().pinned_blocks -= 1;
  live_resources().pinned_bytes -= (int64_t)it->second;
  pin_.erase(it);
}

void HipRes::pfree(void* p) {
  if (!p) return;
  forget(p);
  HIP_OK(hipHostFree(p));
}

void* HipRes::device_alias(const void* pinned_host) {
  void* d = nullptr;
  HIP_OK(hipHostGetDevicePointer(&d, const_cast<void*>(pinned_host), 0));
  return d;
}

hipEvent_t HipRes::new_event() {
  hipEvent_t e = nullptr;
  HIP_OK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  std::lock_guard<std::mutex> g(mu_);
  events_.push_back(e);
  live_resources().events += 1;
  return e;
}

hipStream_t HipRes::adopt(hipStream_t s) {
  std::lock_guard<std::mutex> g(mu_);
  streams_.push_back(s);
  live_resources().streams += 1;
  return s;
}

// Teardown: errors are ignored (the device may already be gone at interpreter exit).
void HipRes::release_all() {
  std::lock_guard<std::mutex> g(mu_);
  LiveResources& L = live_resources();
  for (hipEvent_t e : events_) (void)hipEventDestroy(e);
  L.events -= (int64_t)events_.size();
  events_.clear();
  for (auto& kv : pin_) {
    (void)hipHostFree(kv.first);
    L.pinned_bytes -= (int64_t)kv.second;
  }
  L.pinned_blocks -= (int64_t)pin_.size();
  pin_.clear();
  for (auto& kv : dev_) {
    (void)hipFree(kv.first);
    L.device_bytes -= (int64_t)kv.second;
  }
  L.device_blocks -= (int64_t)dev_.size();
  dev_.clear();
  device_bytes_ = 0;
  for (hipStream_t s : streams_) (void)hipStreamDestroy(s);
  L.streams -= (int64_t)streams_.size();
  streams_.clear();
}

}  // namespace apm
