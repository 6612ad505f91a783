// census.hip — MI355X (gfx950) kernels + C ABI (include/mmsbm.h, mmsbm_census_*, mmsbm_scan_census)
// of the score census: for M sorted thresholds, the exact number of eligible triples (the scan's:
// rank positions a < b < c < P, packed key not among the known ones) whose score is at or above each,
// and the number of eligible triples in all.
//
// The score phase is the scan's (scan_score.h: the same prep, W rows, MFMA chain per tile and, for
// the ensemble, the same slot-order sum and division), so a score carries the same bits here as in
// scan_kernel.  What differs is what happens to a tile of scores:
//
// Binning.  The workgroup holds the thresholds and M + 1 counters in LDS; counter i counts the
// eligible scores with exactly i thresholds at or below them (counter 0: below all).  A lane also
// keeps a private count of its eligible scores below thresholds[0].  One ballot decides whether a
// tile has any eligible score at or above thresholds[0]; when it has none (with thresholds high in
// the distribution, nearly every tile) the lanes add their eligible scores to their private counts
// and the tile is done.  Otherwise a lane finds each such score's counter by a fixed-length binary
// search over the LDS thresholds and adds 1 with an LDS atomic (when every lane of the wave lands on
// one counter, one lane adds the wave's count instead).
//
// Eligibility and exclusion are the sweep's (scan_sweep.h), shared with the pair census.
//
// Counters.  Everything is an integer add: LDS atomics inside the workgroup, at its end one 64-bit
// global atomic add per nonzero counter into a row zeroed by the call, then census_finish_kernel
// forms the suffix sums ("at or above") and the total.  No floating-point value is summed across
// lanes or workgroups, so the counts do not depend on the grid, the batch or the arrival order.

#include <hip/hip_runtime.h>

#include <cstdint>

#include "mmsbm.h"
#include "scan_host.h"
#include "scan_score.h"
#include "scan_sweep.h"

namespace {

using namespace scan_host;
using namespace scan_sweep;
using scan_score::scan_prep_kernel;
using scan_score::Score;
using scan_score::W_LDS_MAX;

constexpr int CENSUS_MAX_M = 1024;  // documented cap of M (include/mmsbm.h)

// Every counter (a lane's, a workgroup's, the global row, the result) is an unsigned 64-bit integer
// and counts triples of one call: at most C(P, 3) < P^3 / 6 <= (2 10^6)^3 / 6 < 1.4 10^18 < 2^63
// (make_plan refuses P > 2 10^6), so none can wrap.
typedef unsigned long long count_t;

struct CensusArgs : SweepArgs {
  const double* thresholds; // [M], non-decreasing
  count_t* bins;            // [M + 1], zeroed: bins[i] = eligible scores with i thresholds at or below
  int M;
};

// The masked census (mmsbm_scan_census_masked): the pair mask travels in the masked kernels' own
// argument struct, so CensusArgs and the unmasked kernels are what they were.
struct CensusMaskedArgs : CensusArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

// At most 4 waves per SIMD, which is what the grid is sized for (sweep_grid): aiming at a fifth, the
// compiler issues the ensemble's operand loads one at a time (measured: 6.51 ms against 5.68 ms at
// P = 1500, K = 10, B = 8).  The cap and sweep_grid's 4 workgroups per compute unit change together:
// a larger default grid could not be resident under this cap, and no instantiation may take a fifth
// wave however few registers it needs.  With a grid set through MMSBM_CENSUS_GRID the cap has not
// been measured.
// The body of both kernels; MASK: Args is CensusMaskedArgs and row a of the mask lies behind the bitmap.
template <int KS, bool ENS, bool MASK, class Args>
__device__ __forceinline__ void census_body(const Args& A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Head* st = reinterpret_cast<Head*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Head));
  const int M = A.M;
  double* thr = W + (size_t)A.ns * 16 * A.WB * Score<KS>::WS;  // [M]
  count_t* cnt = reinterpret_cast<count_t*>(thr + M);          // [M + 1]
  unsigned* bm = reinterpret_cast<unsigned*>(cnt + M + 1);     // [BM_WORDS]

  for (int i = threadIdx.x; i < M; i += NT) thr[i] = A.thresholds[i];
  for (int i = threadIdx.x; i <= M; i += NT) cnt[i] = 0;
  sweep_begin(st);

  const int lane = threadIdx.x & 63;
  const double thr0 = M > 0 ? A.thresholds[0] : __builtin_huge_val();  // M = 0: everything is "below all"
  int top = 1;  // the binary search's first step: the largest power of two <= max(M, 1)
  while (2 * top <= M) top <<= 1;
  count_t below = 0;  // this lane's eligible scores below thresholds[0]

  // Count one finished tile; nothing here depends on the item.
  auto count_tile = [&](int, const d4v& tot, const bool (&el)[4]) {
    // nearly every tile ends here when the thresholds sit high in the distribution
    if (!__ballot((el[0] && tot[0] >= thr0) || (el[1] && tot[1] >= thr0) || (el[2] && tot[2] >= thr0) ||
                  (el[3] && tot[3] >= thr0))) {
      below += (count_t)((int)el[0] + (int)el[1] + (int)el[2] + (int)el[3]);
      return;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double s = tot[i];
      const bool in = el[i] && s >= thr0;
      if (el[i] && !in) ++below;
      // pos = the number of thresholds at or below s (thresholds are non-decreasing); >= 1 for `in`
      int pos = 0;
      for (int step = top; step > 0; step >>= 1)
        if (in && pos + step <= M && thr[pos + step - 1] <= s) pos += step;
      const unsigned long long mk = __ballot(in);
      if (!mk) continue;
      const int first = __shfl(pos, __ffsll((long long)mk) - 1, 64);
      if (!__ballot(in && pos != first)) {  // one counter for the whole wave: one add
        if (lane == 0) atomicAdd(&cnt[first], (count_t)__popcll(mk));
      } else if (in) {
        atomicAdd(&cnt[pos], (count_t)1);
      }
    }
  };
  if constexpr (MASK)
    sweep_masked<KS, ENS>(A, st, W, bm, A.mask, A.MW, bm + BM_WORDS, [&](int, int) { return count_tile; });
  else
    sweep<KS, ENS>(A, st, W, bm, [&](int, int) { return count_tile; });
  if (below) atomicAdd(&cnt[0], below);
  __syncthreads();
  for (int i = threadIdx.x; i <= M; i += NT) {
    const count_t v = cnt[i];
    if (v) __hip_atomic_fetch_add(&A.bins[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <int KS, bool ENS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, 4))) void census_kernel(CensusArgs A) {
  census_body<KS, ENS, false>(A);
}

template <int KS, bool ENS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(1, 4))) void census_masked_kernel(
    CensusMaskedArgs A) {
  census_body<KS, ENS, true>(A);
}

// out[m] = sum of bins[m + 1 .. M] for m < M (the eligible scores at or above thresholds[m]);
// out[M] = sum of bins[0 .. M] (the eligible triples).  One workgroup.
__global__ __launch_bounds__(NT) void census_finish_kernel(const count_t* __restrict__ bins, int M,
                                                           long long* __restrict__ out) {
  __shared__ count_t part[NT];
  const int n = M + 1, per = (n + NT - 1) / NT;
  const int i0 = min((int)threadIdx.x * per, n), i1 = min(i0 + per, n);
  count_t sum = 0;
  for (int i = i0; i < i1; ++i) sum += bins[i];
  part[threadIdx.x] = sum;
  __syncthreads();
  count_t after = 0;  // the bins behind this thread's chunk
  for (int t = threadIdx.x + 1; t < NT; ++t) after += part[t];
  for (int i = i1 - 1; i >= i0; --i) {
    if (i < M) out[i] = (long long)after;  // bins[i + 1 .. M]
    after += bins[i];
  }
  if (threadIdx.x == 0) out[M] = (long long)after;  // thread 0's chunk starts at bin 0
}

struct CensusPlan {
  ScanShape sh;
  size_t off_thT, off_T, off_bins, total;
};

// The workspace follows the context's shape and M only, so one workspace serves every call of that
// shape with at most that many thresholds.
int make_plan(const mmsbm_ctx* c, int M, CensusPlan* p) {
  if (int rc = scan_shape(c, "census", &p->sh)) return rc;
  if (M < 0) return fail(MMSBM_ERR_INVALID, "M=%d < 0", M);
  if (M > CENSUS_MAX_M) return fail(MMSBM_ERR_UNSUPPORTED, "M=%d above the census's cap of %d", M, CENSUS_MAX_M);
  if (int rc = packed_keys_fit(p->sh)) return rc;
  size_t off = 256;
  score_workspace(p->sh, off, &p->off_thT, &p->off_T);
  p->off_bins = off, off = align256(off + sizeof(count_t) * ((size_t)M + 1));
  p->total = off;
  return MMSBM_OK;
}

// Both entry points; `masked`: mmsbm_scan_census_masked, whose mask must not be null.
int census_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
                bool masked, const double* theta, const double* pr, int32_t sample, const double* thresholds,
                int32_t M, void* ws, int64_t ws_bytes, int64_t* out_counts, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  CensusPlan p;
  int rc = make_plan(c, M, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  if (!order || !theta || !pr || !out_counts || (M > 0 && !thresholds))
    return fail(MMSBM_ERR_INVALID, "null pointer");
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "census", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "census", "mmsbm_census_workspace_bytes", known, n_known, sample, ws, ws_bytes, p.total,
                       &ns, &s0)))
    return rc;
  if ((rc = pick_wb(sh, "census", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  const int lds = (int)(sizeof(Head) + w_bytes + sizeof(double) * M + sizeof(count_t) * (M + 1) +
                        sizeof(unsigned) * (BM_WORDS + MW));
  const int G = sweep_grid(sh, WB, "MMSBM_CENSUS_GRID");

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  count_t* bins = (count_t*)(w + p.off_bins);
  HIP_TRY(hipMemsetAsync(bins, 0, sizeof(count_t) * ((size_t)M + 1), s));
  if (sh.P >= 3) {
    scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                     (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P, sh.P16, s0);
    HIP_TRY(hipGetLastError());
    const CensusArgs a{{(const double*)(w + p.off_thT), (const double*)(w + p.off_T), (const long long*)known,
                        n_known, sh.K, sh.P, sh.P16, ns, WB},
                       thresholds, bins, M};
    const CensusMaskedArgs am{a, mask, MW};
    rc = dispatch_ks(sh.KP / 4, [&](auto ks) {
      constexpr int KS = decltype(ks)::value;
      if (masked)
        return ns > 1 ? launch_lds(census_masked_kernel<KS, true>, G, lds, s, am)
                      : launch_lds(census_masked_kernel<KS, false>, G, lds, s, am);
      return ns > 1 ? launch_lds(census_kernel<KS, true>, G, lds, s, a) : launch_lds(census_kernel<KS, false>, G, lds, s, a);
    });
    if (rc) return rc;
  }
  census_finish_kernel<<<1, NT, 0, s>>>(bins, M, (long long*)out_counts);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

}  // namespace

extern "C" {

int mmsbm_census_max_m(void) { return CENSUS_MAX_M; }

int mmsbm_pair_mask_shape(const mmsbm_ctx* c, int32_t* rows, int32_t* words_per_row) {
  if (!c || !rows || !words_per_row) return fail(MMSBM_ERR_INVALID, "null argument");
  ScanShape sh;
  int MW;
  if (int rc = scan_shape(c, "the pair mask", &sh)) return rc;
  if (int rc = pair_mask_words(sh, "the pair mask", &MW)) return rc;
  *rows = sh.P16, *words_per_row = MW;
  return MMSBM_OK;
}

int mmsbm_census_workspace_bytes(const mmsbm_ctx* c, int32_t M, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  CensusPlan p;
  int rc = make_plan(c, M, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_scan_census(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                      const double* theta, const double* pr, int32_t sample, const double* thresholds,
                      int32_t M, void* ws, int64_t ws_bytes, int64_t* out_counts, void* stream) {
  return census_call(c, order, known, n_known, nullptr, false, theta, pr, sample, thresholds, M, ws, ws_bytes,
                     out_counts, stream);
}

int mmsbm_scan_census_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                             const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                             const double* thresholds, int32_t M, void* ws, int64_t ws_bytes,
                             int64_t* out_counts, void* stream) {
  return census_call(c, order, known, n_known, mask, true, theta, pr, sample, thresholds, M, ws, ws_bytes,
                     out_counts, stream);
}

}  // extern "C"
