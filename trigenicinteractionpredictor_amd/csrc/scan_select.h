// scan_select.h — the selection machinery shared by the genome-wide scan (scan.hip) and the partner
// scan (partners.hip): the total order, a workgroup's candidate buffer with ballot-compacted
// appends, keep-best-N by a bitonic sort and the list merge; and the sorted known-key search
// (lower_bound, is_known), which the census sweep (scan_sweep.h) uses too.  Device code only: the
// host side of every family is scan_host.h.
//
// Every entry of a buffer is (score, key); the total order is score descending, key ascending, so
// the best N of any set is unique and does not depend on who appended what when.  Everything is
// inline or static: each translation unit pulls it in with `using namespace scan_select`.
#ifndef MMSBM_SCAN_SELECT_H
#define MMSBM_SCAN_SELECT_H

#include <hip/hip_runtime.h>

#include <climits>

namespace scan_select {

constexpr int NT = 256;  // threads per workgroup of every scan kernel
constexpr int FAN = 32;  // lists merged by one workgroup of a merge kernel
constexpr int LDS_MAX = 144 * 1024;

typedef double d4v __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// Selection state of one workgroup (LDS) and its candidate buffer
// ------------------------------------------------------------------------------------------
struct Sel {
  int count;        // entries in the buffer
  int overflow;     // a wave's reservation did not fit: sort and keep the best N
  double thr_s;     // the workgroup's N-th best (score, key); (-inf, max) until it has N
  long long thr_k;
  double gthr;      // the published bound as read at the item's start (-inf: none)
  long long klo, khi;  // the item's known keys are known[klo, khi)
  double pad[2];
};
static_assert(sizeof(Sel) == 64, "Sel is the first 64 bytes of the dynamic LDS");

__device__ __forceinline__ double neg_inf() { return -__builtin_huge_val(); }

// the total order: score descending, packed key ascending
__device__ __forceinline__ bool before(double s1, long long k1, double s2, long long k2) {
  return s1 > s2 || (s1 == s2 && k1 < k2);
}

__device__ __forceinline__ void sel_init(Sel* st) {
  st->count = 0;
  st->overflow = 0;
  st->thr_s = neg_inf();
  st->thr_k = LLONG_MAX;
  st->gthr = neg_inf();
  st->klo = st->khi = 0;
}

// Reserve n entries for this wave (lane 0, one LDS compare-exchange); -1: no room, nothing taken.
__device__ __forceinline__ int wave_reserve(Sel* st, int n, int cap) {
  int base = 0;
  if ((threadIdx.x & 63) == 0) {
    int old = __hip_atomic_load(&st->count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    for (;;) {
      if (old + n > cap) {
        old = -1;
        __hip_atomic_store(&st->overflow, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        break;
      }
      if (__hip_atomic_compare_exchange_strong(&st->count, &old, old + n, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
        break;
    }
    base = old;
  }
  return __shfl(base, 0, 64);
}

// Sort the buffer under the total order, keep the best N, raise the threshold.  Called by the
// whole workgroup; begins and ends with a barrier.
// Inlined, so that a buffer in LDS is sorted with LDS instructions (the address space is inferred).
__device__ __forceinline__ void wg_keep_best(Sel* st, double* cs, long long* ck, int N,
                                             unsigned long long* shared) {
  __syncthreads();
  const int cnt = st->count;
  int sz = 1;
  while (sz < cnt) sz <<= 1;
  for (int i = cnt + threadIdx.x; i < sz; i += NT) {
    cs[i] = neg_inf();
    ck[i] = LLONG_MAX;
  }
  __syncthreads();
  for (int k = 2; k <= sz; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (sz >> 1); t += NT) {  // one compare-exchange per pair (i, i + j)
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), x = i | j;
        const double si = cs[i], sx = cs[x];
        const long long ki = ck[i], kx = ck[x];
        const bool up = (i & k) == 0;
        if (up ? before(sx, kx, si, ki) : before(si, ki, sx, kx)) {
          cs[i] = sx;
          ck[i] = kx;
          cs[x] = si;
          ck[x] = ki;
        }
      }
      __syncthreads();
    }
  }
  if (threadIdx.x == 0) {
    const int keep = cnt < N ? cnt : N;
    st->count = keep;
    st->overflow = 0;
    if (keep == N) {
      const double t = cs[N - 1];
      st->thr_s = t;
      st->thr_k = ck[N - 1];
      if (shared && t > 0.0)
        __hip_atomic_fetch_max(shared, (unsigned long long)__double_as_longlong(t), __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  __syncthreads();
}

// Merge the sorted lists [l0, l1) of in_s / in_k [.][N] (in_n entries each) into the workgroup's
// buffer, keeping the best N whenever it fills.  Called by the whole workgroup after sel_init and
// a barrier; the caller ends with wg_keep_best.
__device__ __forceinline__ void wg_merge_lists(Sel* st, double* cs, long long* ck,
                                               const double* __restrict__ in_s,
                                               const long long* __restrict__ in_k,
                                               const int* __restrict__ in_n, int l0, int l1, int N,
                                               int cap) {
  const int lane = threadIdx.x & 63;
  for (int l = l0; l < l1; ++l) {
    const int cnt = min(in_n[l], N);
    for (int base = 0; base < cnt; base += NT) {
      const int i = base + threadIdx.x;
      double s = 0.0;
      long long k = 0;
      bool pass = false;
      if (i < cnt) {
        s = in_s[(size_t)l * N + i];
        k = in_k[(size_t)l * N + i];
        pass = before(s, k, *(volatile double*)&st->thr_s, *(volatile long long*)&st->thr_k);
      }
      bool done = false;
      for (;;) {
        if (!done) {
          const unsigned long long mk = __ballot(pass);
          const int n = __popcll(mk);
          int pos = n ? wave_reserve(st, n, cap) : 0;
          if (pos >= 0) {
            if (pass) {
              pos += __popcll(mk & ((1ull << lane) - 1ull));
              cs[pos] = s;
              ck[pos] = k;
            }
            done = true;
          }
        }
        __syncthreads();
        const int full = st->overflow;
        __syncthreads();  // everyone has read the flag before the next chunk can raise it
        if (!full) break;
        wg_keep_best(st, cs, ck, N, nullptr);
      }
    }
  }
}

// first index in known[lo, hi) whose key is not below `key`
__device__ __forceinline__ long long lower_bound(const long long* __restrict__ known, long long lo,
                                                 long long hi, long long key) {
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (known[mid] < key) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool is_known(const long long* __restrict__ known, long long lo, long long hi,
                                         long long key) {
  const long long at = lower_bound(known, lo, hi, key);
  return at < hi && known[at] == key;
}

}  // namespace scan_select

#endif  // MMSBM_SCAN_SELECT_H
