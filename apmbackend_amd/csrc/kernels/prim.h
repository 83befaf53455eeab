// rocPRIM's device-wide primitives, each call written once.  rocPRIM wants every call twice: with
// a null scratch pointer to learn the bytes it needs, then with the scratch.  The wrappers below do
// both from one argument list, so the size query, the capacity check and the run cannot disagree on
// types, config or bit range -- and the *_tmp_bytes sizing functions call the same wrappers with
// null data pointers instead of keeping a copy of that list.
#pragma once
#include <algorithm>
#include <rocprim/rocprim.hpp>

#include "common.h"

namespace apm {

// The scratch a launcher was given.  A default-constructed one makes every wrapper a size query
// only (nothing is launched); `need` keeps the largest requirement seen, which is what a sizing
// function returns.
struct PrimScratch {
  PrimScratch() = default;
  PrimScratch(void* tmp_, size_t cap_) : tmp(tmp_), cap(cap_), size_only(false) {}
  void* tmp = nullptr;
  size_t cap = 0;
  size_t need = 0;
  bool size_only = true;
};

// call(tmp, bytes) -> hipError_t is one rocPRIM call.  0: ran (or sized); -1: the scratch is too
// small and nothing was launched.  A HIP error aborts, as everywhere in the launchers.
template <class Call>
inline int prim_call(PrimScratch& sc, Call&& call) {
  size_t need = 0;
  HIP_OK(call(nullptr, need));
  sc.need = std::max(sc.need, need);
  if (sc.size_only) return 0;
  if (need > sc.cap) return -1;
  HIP_OK(call(sc.tmp, need));
  return 0;
}

template <class In, class Out, class Init, class Op>
inline int prim_exclusive_scan(PrimScratch& sc, In in, Out out, Init init, size_t n, Op op, hipStream_t s) {
  return prim_call(sc, [&](void* t, size_t& b) { return rocprim::exclusive_scan(t, b, in, out, init, n, op, s); });
}

template <class In, class Out, class Op>
inline int prim_inclusive_scan(PrimScratch& sc, In in, Out out, size_t n, Op op, hipStream_t s) {
  return prim_call(sc, [&](void* t, size_t& b) { return rocprim::inclusive_scan(t, b, in, out, n, op, s); });
}

// all key bits, default config
template <class K, class V>
inline int prim_sort_pairs(PrimScratch& sc, const K* k_in, K* k_out, const V* v_in, V* v_out, size_t n, hipStream_t s) {
  return prim_call(sc, [&](void* t, size_t& b) {
    return rocprim::radix_sort_pairs(t, b, k_in, k_out, v_in, v_out, n, 0, 8 * sizeof(K), s);
  });
}

template <class K, class V, class Off>
inline int prim_segmented_sort_pairs(PrimScratch& sc, const K* k_in, K* k_out, const V* v_in, V* v_out, size_t n,
                                     unsigned segments, Off seg_begin, Off seg_end, unsigned bit_lo, unsigned bit_hi,
                                     hipStream_t s) {
  return prim_call(sc, [&](void* t, size_t& b) {
    return rocprim::segmented_radix_sort_pairs(t, b, k_in, k_out, v_in, v_out, n, segments, seg_begin, seg_end, bit_lo,
                                               bit_hi, s);
  });
}

// (keys_a, vals_a) and (keys_b, vals_b), each sorted -> (keys_out, vals_out); stable, a first on ties
template <class K, class V, class Cmp>
inline int prim_merge(PrimScratch& sc, const K* k_a, const K* k_b, K* k_out, const V* v_a, const V* v_b, V* v_out,
                      size_t n_a, size_t n_b, Cmp cmp, hipStream_t s) {
  return prim_call(sc, [&](void* t, size_t& b) {
    return rocprim::merge(t, b, k_a, k_b, k_out, v_a, v_b, v_out, n_a, n_b, cmp, s);
  });
}

template <class In, class Out, class Count, class Pred>
inline int prim_select(PrimScratch& sc, In in, Out out, Count d_count, size_t n, Pred pred, hipStream_t s) {
  return prim_call(sc, [&](void* t, size_t& b) { return rocprim::select(t, b, in, out, d_count, n, pred, s); });
}

}  // namespace apm
