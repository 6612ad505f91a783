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
// Exclusion.  Per item (a, row block) two searches bound the known keys whose first two positions
// fall into the item: known[lo, hi).  The workgroup sets one bit per (b-tile, c-tile mod CT_BITS)
// that holds one of them in an LDS bitmap; is_known runs only for the lanes of flagged tiles, over
// [lo, hi).  A c-tile index beyond CT_BITS shares a bit with another: a flag may be set for a tile
// without known keys, which costs searches and nothing else.
//
// Counters.  Everything is an integer add: LDS atomics inside the workgroup, at its end one 64-bit
// global atomic add per nonzero counter into a row zeroed by the call, then census_finish_kernel
// forms the suffix sums ("at or above") and the total.  No floating-point value is summed across
// lanes or workgroups, so the counts do not depend on the grid, the batch or the arrival order.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "mmsbm.h"
#include "scan_score.h"
#include "scan_select.h"

namespace {

using namespace scan_select;
using scan_score::pick_wb;
using scan_score::scan_prep_kernel;
using scan_score::Score;
using scan_score::W_LDS_MAX;

constexpr int CENSUS_MAX_M = 1024;  // documented cap of M (include/mmsbm.h)
constexpr int CT_BITS = 2048;       // c-tile bits per b-tile of the exclusion bitmap
constexpr int BM_WORDS = 4 * CT_BITS / 32;
constexpr int GRID_MAX = 1 << 20;

// Every counter (a lane's, a workgroup's, the global row, the result) is an unsigned 64-bit integer
// and counts triples of one call: at most C(P, 3) < P^3 / 6 <= (2 10^6)^3 / 6 < 1.4 10^18 < 2^63
// (make_plan refuses P > 2 10^6), so none can wrap.
typedef unsigned long long count_t;

struct CensusHead {        // the first 64 bytes of the dynamic LDS
  long long lo, hi;        // the item's known keys are known[lo, hi)
  long long pad[6];
};
static_assert(sizeof(CensusHead) == 64, "CensusHead is the first 64 bytes of the dynamic LDS");

struct CensusArgs {
  const double* thT;        // [ns][KP][P16]
  const double* T;          // [ns][P][K][KP]
  const long long* known;   // sorted packed keys (null: none)
  long long n_known;
  const double* thresholds; // [M], non-decreasing
  count_t* bins;            // [M + 1], zeroed: bins[i] = eligible scores with i thresholds at or below
  int K, P, P16, ns, M, WB;
};

template <int KS>
__global__ __launch_bounds__(NT) void census_kernel(CensusArgs A) {
  using Sc = Score<KS>;  // the score phase (scan_score.h)
  constexpr int WS = Sc::WS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  CensusHead* st = reinterpret_cast<CensusHead*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(CensusHead));
  const int RB = 16 * A.WB;  // rows b of one item
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns, M = A.M;
  double* thr = W + (size_t)ns * RB * WS;                    // [M]
  count_t* cnt = reinterpret_cast<count_t*>(thr + M);        // [M + 1]
  unsigned* bm = reinterpret_cast<unsigned*>(cnt + M + 1);   // [BM_WORDS]

  for (int i = threadIdx.x; i < M; i += NT) thr[i] = A.thresholds[i];
  for (int i = threadIdx.x; i <= M; i += NT) cnt[i] = 0;
  if (threadIdx.x == 0) st->lo = st->hi = 0;
  __syncthreads();

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const long long PP = (long long)P;
  const double div = (double)ns;
  const bool has_known = A.n_known > 0;
  const double thr0 = M > 0 ? A.thresholds[0] : __builtin_huge_val();  // M = 0: everything is "below all"
  int top = 1;  // the binary search's first step: the largest power of two <= max(M, 1)
  while (2 * top <= M) top <<= 1;
  count_t below = 0;  // this lane's eligible scores below thresholds[0]

  // items round-robin over the workgroups, skipped exactly as the scan skips them
  for (long long q = blockIdx.x; q < PP * nbq; q += gridDim.x) {
    const int a = (int)(q / nbq), bq = (int)(q % nbq);
    if (a >= P - 2 || bq * RB + RB - 1 <= a || bq * RB >= P - 1) continue;  // no a < b < c here
    __syncthreads();  // the previous item's W, bitmap and range are read
    if (has_known) {
      // the known keys whose first position is a and whose second falls into the item's rows
      if (threadIdx.x == 64) st->lo = lower_bound(A.known, 0, A.n_known, ((long long)a * PP + (long long)bq * RB) * PP);
      if (threadIdx.x == 128)
        st->hi = lower_bound(A.known, 0, A.n_known, ((long long)a * PP + (long long)bq * RB + RB) * PP);
      for (int i = threadIdx.x; i < BM_WORDS; i += NT) bm[i] = 0;
    }
    Sc::fill_w(W, A.T, A.thT, a, bq, RB, ns, K, P, P16);  // W_a of the item's rows, every sample
    __syncthreads();
    const long long klo = st->lo, khi = st->hi;
    if (khi > klo) {  // workgroup-uniform
      for (long long i = klo + threadIdx.x; i < khi; i += NT) {
        const long long key = A.known[i];
        const int tb = (int)((key / PP) % PP) / 16 - bq * A.WB, tc = (int)(key % PP) / 16;
        if (tb >= 0 && tb < A.WB)  // always: [klo, khi) holds the item's rows only
          atomicOr(&bm[tb * (CT_BITS / 32) + ((tc & (CT_BITS - 1)) >> 5)], 1u << (tc & 31));
      }
      __syncthreads();
    }

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1 && b0 + 15 > a;
    if (!wave_on) continue;
    double areg[KS];
    if (ns == 1) Sc::load_a(areg, W, wb, m, kk);
    int ct = bq * A.WB + wc;
    while (ct < btile) ct += CW;  // every c of those tiles is below every b
    double bnext[KS];  // single sample: the next tile's Th' operand is in flight
    if (ns == 1 && ct < nct) Sc::load_b(bnext, A.thT, P16, ct * 16, m, kk);
    // Count one finished tile: lane holds S[b0 + kk + 4 i][c0 + m] in tot[i].
    auto count_tile = [&](const d4v& tot, int ct) {
      const int c0 = ct * 16, c = c0 + m;
      bool el[4];  // el[i]: that triple is eligible
      if (b0 > a && c0 > b0 + 15 && c0 + 16 <= P) {  // an interior tile: a < b < c < P everywhere
        el[0] = el[1] = el[2] = el[3] = true;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int b = b0 + kk + 4 * i;
          el[i] = a < b && b < c && c < P;
        }
      }
      if (khi > klo && ((bm[wb * (CT_BITS / 32) + ((ct & (CT_BITS - 1)) >> 5)] >> (ct & 31)) & 1u)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long key = ((long long)a * PP + (b0 + kk + 4 * i)) * PP + c;
          if (el[i]) el[i] = !is_known(A.known, klo, khi, key);
        }
      }
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
    // A tile is counted after the next tile's MFMA chain has been issued, so the counting code does
    // not depend on the newest accumulator (measured: 12 % off the B = 8 ensemble, nothing at B = 1).
    d4v prev = {0.0, 0.0, 0.0, 0.0};
    int prev_ct = -1;
    for (; ct < nct; ct += CW) {
      const int c0 = ct * 16;
      d4v tot;
      if (ns == 1) {
        double bcur[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
        if (ct + CW < nct) Sc::load_b(bnext, A.thT, P16, c0 + 16 * CW, m, kk);
        tot = Sc::tile_one(areg, bcur);
      } else {
        tot = Sc::tile_mean(W, A.thT, ns, RB, P16, wb, c0, m, kk, div);
      }
      if (prev_ct >= 0) count_tile(prev, prev_ct);
      prev = tot;
      prev_ct = ct;
    }
    if (prev_ct >= 0) count_tile(prev, prev_ct);
  }
  if (below) atomicAdd(&cnt[0], below);
  __syncthreads();
  for (int i = threadIdx.x; i <= M; i += NT) {
    const count_t v = cnt[i];
    if (v) __hip_atomic_fetch_add(&A.bins[i], v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
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
  int device, K, KP, R, B, P, P16, nact, ncu;
  size_t off_thT, off_T, off_bins, total;
};

// The workspace follows the context's shape and M only, so one workspace serves every call of that
// shape with at most that many thresholds.
int make_plan(const mmsbm_ctx* c, int M, CensusPlan* p) {
  mmsbm_detail_scan_shape(c, &p->device, &p->K, &p->R, &p->B, &p->P, &p->nact, &p->ncu);
  if (p->K < 1 || p->K > MMSBM_MAX_K)
    return fail(MMSBM_ERR_UNSUPPORTED, "K=%d outside [1, %d]: call mmsbm_set_shape", p->K, MMSBM_MAX_K);
  if (p->R < 2 || p->B < 1 || p->P < 0) return fail(MMSBM_ERR_INVALID, "census needs R >= 2, B >= 1 (mmsbm_set_shape)");
  if (M < 0) return fail(MMSBM_ERR_INVALID, "M=%d < 0", M);
  if (M > CENSUS_MAX_M) return fail(MMSBM_ERR_UNSUPPORTED, "M=%d above the census's cap of %d", M, CENSUS_MAX_M);
  if ((long long)p->P > 2000000) return fail(MMSBM_ERR_UNSUPPORTED, "P=%d: packed keys overflow", p->P);
  p->KP = (p->K + 3) / 4 * 4;
  p->P16 = std::max(16, (p->P + 15) / 16 * 16);
  const size_t B = p->B, P = p->P, K = p->K, KP = p->KP, P16 = p->P16;
  size_t off = 256;
  p->off_thT = off, off = align256(off + sizeof(double) * B * KP * P16);
  p->off_T = off, off = align256(off + sizeof(double) * B * P * K * KP);
  p->off_bins = off, off = align256(off + sizeof(count_t) * ((size_t)M + 1));
  p->total = off;
  return MMSBM_OK;
}

template <int KS>
int launch_census(const CensusArgs& a, int G, int lds, hipStream_t s) {
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&census_kernel<KS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  census_kernel<KS><<<G, NT, lds, s>>>(a);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

}  // namespace

extern "C" {

int mmsbm_census_max_m(void) { return CENSUS_MAX_M; }

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
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  CensusPlan p;
  int rc = make_plan(c, M, &p);
  if (rc) return rc;
  if (!order || !theta || !pr || !out_counts || (M > 0 && !thresholds))
    return fail(MMSBM_ERR_INVALID, "null pointer");
  if (n_known < 0 || (n_known > 0 && !known)) return fail(MMSBM_ERR_INVALID, "bad known-key table");
  if (sample < -1 || sample >= p.nact)
    return fail(MMSBM_ERR_INVALID, "sample %d outside the active prefix [0, %d)", sample, p.nact);
  if (!ws || ws_bytes < (int64_t)p.total || ((uintptr_t)ws & 15))
    return fail(MMSBM_ERR_INVALID, "census workspace missing, misaligned or too small (mmsbm_census_workspace_bytes)");
  const int ns = sample >= 0 ? 1 : p.nact, s0 = sample >= 0 ? sample : 0;
  size_t w_bytes = 0;
  const int WB = pick_wb(ns, p.KP, &w_bytes);
  if (w_bytes > (size_t)W_LDS_MAX)
    return fail(MMSBM_ERR_UNSUPPORTED, "an ensemble of %d samples at K=%d exceeds the census's LDS tile: count the samples one by one",
                ns, p.K);
  const int lds = (int)(sizeof(CensusHead) + w_bytes + sizeof(double) * M + sizeof(count_t) * (M + 1) +
                        sizeof(unsigned) * BM_WORDS);
  const long long items = std::max<long long>(1, (long long)p.P * ((p.P + 16 * WB - 1) / (16 * WB)));
  long long G = std::min<long long>(4LL * p.ncu, items);
  if (const char* e = getenv("MMSBM_CENSUS_GRID")) {  // measurement: the number of workgroups
    const long long g = atoll(e);
    if (g >= 1) G = std::min<long long>(g, GRID_MAX);
  }

  DeviceGuard g(p.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  count_t* bins = (count_t*)(w + p.off_bins);
  HIP_TRY(hipMemsetAsync(bins, 0, sizeof(count_t) * ((size_t)M + 1), s));
  if (p.P >= 3) {
    scan_prep_kernel<<<dim3(p.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                    (double*)(w + p.off_T), p.K, p.KP, p.R, p.P, p.P16, s0);
    HIP_TRY(hipGetLastError());
    CensusArgs a{};
    a.thT = (const double*)(w + p.off_thT);
    a.T = (const double*)(w + p.off_T);
    a.known = (const long long*)known;
    a.n_known = n_known;
    a.thresholds = thresholds;
    a.bins = bins;
    a.K = p.K, a.P = p.P, a.P16 = p.P16, a.ns = ns, a.M = M, a.WB = WB;
    switch (p.KP / 4) {
      case 1: rc = launch_census<1>(a, (int)G, lds, s); break;
      case 2: rc = launch_census<2>(a, (int)G, lds, s); break;
      case 3: rc = launch_census<3>(a, (int)G, lds, s); break;
      case 4: rc = launch_census<4>(a, (int)G, lds, s); break;
      case 5: rc = launch_census<5>(a, (int)G, lds, s); break;
      case 6: rc = launch_census<6>(a, (int)G, lds, s); break;
      case 7: rc = launch_census<7>(a, (int)G, lds, s); break;
      default: rc = launch_census<8>(a, (int)G, lds, s); break;
    }
    if (rc) return rc;
  }
  census_finish_kernel<<<1, NT, 0, s>>>(bins, M, (long long*)out_counts);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

}  // extern "C"
