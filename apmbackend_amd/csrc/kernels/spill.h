// A series' spilled samples of one bucket slot, shared by K8 (stats.hip) and K15 (hist.hip).
// Before every K8 each slot's spill list is sorted by series (apm_spill_sort), so the samples a
// series has beyond its inline cell are one contiguous run found by binary search.  counts[] holds
// stored samples only (K7 takes a dropped one back out) and the list length is clamped to its
// capacity, which is what keeps run[k - cap], k < count, inside the list.
#pragma once
#include "kernel_api.h"

namespace apm {

// first position of series s in a slot's sorted spill list [0, n)
__device__ __forceinline__ int spill_lower(const int32_t* keys, int n, int32_t s) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < s) lo = mid + 1; else hi = mid;
  }
  return lo;
}
// the run of series s's spilled samples in slot sl: [*first, *first + cnt - cap)
__device__ __forceinline__ const int32_t* spill_run(const StatsState& st, int sl, int s) {
  const size_t base = (size_t)sl * st.spill_cap;
  const int ns = min(st.spill_n[sl], st.spill_cap);
  return st.spill_val + base + spill_lower(st.spill_series + base, ns, s);
}

}  // namespace apm
