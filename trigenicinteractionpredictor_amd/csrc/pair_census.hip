// pair_census.hip — MI355X (gfx950) kernel + C ABI (include/mmsbm.h, mmsbm_pair_census_*) of the
// pair census: for M sorted thresholds and every pair of rank positions x < y, the exact number of
// eligible triples (the scan's: rank positions a < b < c < P, packed key not among the known ones)
// that contain both x and y and whose score is at or above each threshold.
//
// The score phase is the scan's (scan_score.h: the same prep, W rows, MFMA chain per tile and, for
// the ensemble, the same slot-order sum and division), the work items, the item skipping, the
// eligibility tests and the bitmap-guided known-key lookups are the census's (census.hip), so the
// same triples are hits here and there: for every m, the sum of out[x][y][m] over x < y is three
// times the census count at thresholds[m], exactly.
//
// Binning.  A hit is an eligible triple (a, b, c) with score >= thresholds[0]; it belongs to the
// pairs (a, b), (a, c) and (b, c), and to every m with score >= thresholds[m] (the thresholds are
// non-decreasing, so those m form a prefix).  One ballot decides whether a tile has a hit; when it
// has none (with thresholds high in the distribution, nearly every tile) the tile is done.  In a
// tile with hits a lane holds S[b0 + kk + 4 i][c0 + m], so
//   (a, b): the 16 lanes of one kk share a row: one ballot per row counts its hits and one lane
//           issues one add per (row, m) that is nonzero;
//   (a, c): a lane's four elements share column c: they are added in the lane, the four kk groups
//           by two cross-lane moves, and the 16 lanes of kk = 0 issue one add per (column, m);
//   (b, c): one add per hit and m.
// Every add is an integer add: registers, ballots and integer cross-lane moves, and relaxed
// agent-scope 32-bit atomic adds into the output, which the call has zeroed.  No floating-point
// value crosses a lane, so the counts do not depend on the grid, the batch or the arrival order.
// The thresholds sit in LDS and a tile with hits walks them upwards until one has no hit in the
// tile (M <= 8: no search).
//
// Rows are counted per tile and not per sweep.  Counters of the four rows kept in registers over the
// c sweep (4 M of them, reduced once per item) took the kernel to 156 VGPRs at K = 10: 3 workgroups
// per CU instead of the 4 the grid is sized for, and the call with no hit at all ran at 1.23 ms
// against the census's 0.86 ms (P = 1500).  What they would save is small where it matters: at hit
// fractions up to 1 % a row has few hits per sweep to merge, and the (b, c) adds, which nothing can
// merge, are the most in every regime.
//
// Exclusion bookkeeping (known[lo, hi) of the item, one bit per (b-tile, c-tile mod CT_BITS) in an
// LDS bitmap) is the census's, repeated here because census.hip keeps it in its kernel.

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

constexpr int PAIR_MAX_M = 8;       // documented cap of M (include/mmsbm.h)
constexpr int PAIR_MAX_P = 16384;   // documented cap of P: x P + y < 2^28, the output at most 8 GiB
constexpr int CT_BITS = 2048;       // c-tile bits per b-tile of the exclusion bitmap
constexpr int BM_WORDS = 4 * CT_BITS / 32;
constexpr int GRID_MAX = 1 << 20;

struct PairHead {          // the first 64 bytes of the dynamic LDS
  long long lo, hi;        // the item's known keys are known[lo, hi)
  long long pad[6];
};
static_assert(sizeof(PairHead) == 64, "PairHead is the first 64 bytes of the dynamic LDS");

struct PairArgs {
  const double* thT;        // [ns][KP][P16]
  const double* T;          // [ns][P][K][KP]
  const long long* known;   // sorted packed keys (null: none)
  long long n_known;
  const double* thresholds; // [M], non-decreasing, M >= 1
  int* out;                 // [P][P][M], zeroed; only x < y is touched
  int K, P, P16, ns, M, WB;
};

__device__ __forceinline__ void add(int* p, int v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ENS: the ensemble (ns > 1; a single sample otherwise, as the census's ns == 1 paths).  A template
// parameter, so that neither path holds the other's registers: one kernel for both took 132 VGPRs at
// K = 10 against the census's 120, which leaves 3 workgroups per CU of the 4 the grid is sized for;
// split, the single-sample kernel takes 108 and the ensemble's 120.
template <int KS, bool ENS>
__global__ __launch_bounds__(NT) void pair_census_kernel(PairArgs A) {
  using Sc = Score<KS>;  // the score phase (scan_score.h)
  constexpr int WS = Sc::WS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  PairHead* st = reinterpret_cast<PairHead*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(PairHead));
  const int RB = 16 * A.WB;  // rows b of one item
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns, M = A.M;
  unsigned* bm = reinterpret_cast<unsigned*>(W + (size_t)ns * RB * WS);  // [BM_WORDS]
  double* thr = reinterpret_cast<double*>(bm + BM_WORDS);                // [M]

  if (threadIdx.x < M) thr[threadIdx.x] = A.thresholds[threadIdx.x];
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
  const double thr0 = A.thresholds[0];  // M >= 1
  int* const out = A.out;

  // items round-robin over the workgroups, skipped exactly as the scan and the census skip them
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
    if (!ENS) Sc::load_a(areg, W, wb, m, kk);
    int ct = bq * A.WB + wc;
    while (ct < btile) ct += CW;  // every c of those tiles is below every b
    double bnext[KS];  // single sample: the next tile's Th' operand is in flight
    if (!ENS && ct < nct) Sc::load_b(bnext, A.thT, P16, ct * 16, m, kk);
    const size_t rowa = (size_t)a * P;  // out[a][.][.]
    // Bin one finished tile: lane holds S[b0 + kk + 4 i][c0 + m] in tot[i].
    auto bin_tile = [&](const d4v& tot, int ct) {
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
                    (el[3] && tot[3] >= thr0)))
        return;
#pragma nounroll
      for (int t = 0; t < M; ++t) {
        const double th = thr[t];
        unsigned long long hits = 0;  // the wave's hits at or above thr[t]
        int col = 0;                  // this lane's hits of column c at or above thr[t]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool h = el[i] && tot[i] >= th;  // el: a < b < c < P, every index below is in range
          col += (int)h;
          if (h) add(&out[((size_t)(b0 + kk + 4 * i) * P + c) * M + t], 1);  // (b, c)
          // (a, b): lanes 16 kk .. 16 kk + 15 of the ballot hold row b0 + kk + 4 i
          const unsigned long long mk = __ballot(h);
          hits |= mk;
          const int row = __popcll((mk >> (16 * kk)) & 0xffffull);
          if (m == 0 && row) add(&out[(rowa + (b0 + kk + 4 * i)) * M + t], row);  // row > 0 only where a < b < P
        }
        if (!hits) break;  // the thresholds do not decrease: no hit at the later ones either
        col += __shfl_xor(col, 16, 64);
        col += __shfl_xor(col, 32, 64);
        if (kk == 0 && col) add(&out[(rowa + c) * M + t], col);  // (a, c): col > 0 only where c < P
      }
    };
    // A tile is binned after the next tile's MFMA chain has been issued, as the census counts it.
    d4v prev = {0.0, 0.0, 0.0, 0.0};
    int prev_ct = -1;
    for (; ct < nct; ct += CW) {
      const int c0 = ct * 16;
      d4v tot;
      if (!ENS) {
        double bcur[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
        if (ct + CW < nct) Sc::load_b(bnext, A.thT, P16, c0 + 16 * CW, m, kk);
        tot = Sc::tile_one(areg, bcur);
      } else {
        tot = Sc::tile_mean(W, A.thT, ns, RB, P16, wb, c0, m, kk, div);
      }
      if (prev_ct >= 0) bin_tile(prev, prev_ct);
      prev = tot;
      prev_ct = ct;
    }
    if (prev_ct >= 0) bin_tile(prev, prev_ct);
  }
}

struct PairPlan {
  int device, K, KP, R, B, P, P16, nact, ncu;
  size_t off_thT, off_T, total;
};

// The workspace follows the context's shape only (M is checked here and needs no scratch).
int make_plan(const mmsbm_ctx* c, int M, PairPlan* p) {
  mmsbm_detail_scan_shape(c, &p->device, &p->K, &p->R, &p->B, &p->P, &p->nact, &p->ncu);
  if (p->K < 1 || p->K > MMSBM_MAX_K)
    return fail(MMSBM_ERR_UNSUPPORTED, "K=%d outside [1, %d]: call mmsbm_set_shape", p->K, MMSBM_MAX_K);
  if (p->R < 2 || p->B < 1 || p->P < 0)
    return fail(MMSBM_ERR_INVALID, "pair census needs R >= 2, B >= 1 (mmsbm_set_shape)");
  if (M < 0) return fail(MMSBM_ERR_INVALID, "M=%d < 0", M);
  if (M > PAIR_MAX_M) return fail(MMSBM_ERR_UNSUPPORTED, "M=%d above the pair census's cap of %d", M, PAIR_MAX_M);
  if (p->P > PAIR_MAX_P)
    return fail(MMSBM_ERR_UNSUPPORTED, "P=%d above the pair census's cap of %d (a P x P x M matrix)", p->P, PAIR_MAX_P);
  p->KP = (p->K + 3) / 4 * 4;
  p->P16 = std::max(16, (p->P + 15) / 16 * 16);
  const size_t B = p->B, P = p->P, K = p->K, KP = p->KP, P16 = p->P16;
  size_t off = 256;
  p->off_thT = off, off = align256(off + sizeof(double) * B * KP * P16);
  p->off_T = off, off = align256(off + sizeof(double) * B * P * K * KP);
  p->total = off;
  return MMSBM_OK;
}

template <int KS, bool ENS>
int launch_kernel(const PairArgs& a, int G, int lds, hipStream_t s) {
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(&pair_census_kernel<KS, ENS>),
                                hipFuncAttributeMaxDynamicSharedMemorySize, lds));
  pair_census_kernel<KS, ENS><<<G, NT, lds, s>>>(a);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

template <int KS>
int launch_pair_census(const PairArgs& a, int G, int lds, hipStream_t s) {
  return a.ns > 1 ? launch_kernel<KS, true>(a, G, lds, s) : launch_kernel<KS, false>(a, G, lds, s);
}

}  // namespace

extern "C" {

int mmsbm_pair_census_max_m(void) { return PAIR_MAX_M; }

int mmsbm_pair_census_workspace_bytes(const mmsbm_ctx* c, int32_t M, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  PairPlan p;
  int rc = make_plan(c, M, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_pair_census(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                      const double* theta, const double* pr, int32_t sample, const double* thresholds,
                      int32_t M, void* ws, int64_t ws_bytes, int32_t* out_counts, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  PairPlan p;
  int rc = make_plan(c, M, &p);
  if (rc) return rc;
  if (!order || !theta || !pr || (M > 0 && (!thresholds || !out_counts)))
    return fail(MMSBM_ERR_INVALID, "null pointer");
  if (n_known < 0 || (n_known > 0 && !known)) return fail(MMSBM_ERR_INVALID, "bad known-key table");
  if (sample < -1 || sample >= p.nact)
    return fail(MMSBM_ERR_INVALID, "sample %d outside the active prefix [0, %d)", sample, p.nact);
  if (!ws || ws_bytes < (int64_t)p.total || ((uintptr_t)ws & 15))
    return fail(MMSBM_ERR_INVALID,
                "pair census workspace missing, misaligned or too small (mmsbm_pair_census_workspace_bytes)");
  const int ns = sample >= 0 ? 1 : p.nact, s0 = sample >= 0 ? sample : 0;
  size_t w_bytes = 0;
  const int WB = pick_wb(ns, p.KP, &w_bytes);
  if (w_bytes > (size_t)W_LDS_MAX)
    return fail(MMSBM_ERR_UNSUPPORTED,
                "an ensemble of %d samples at K=%d exceeds the pair census's LDS tile: count the samples one by one", ns,
                p.K);
  if (M == 0) return MMSBM_OK;  // an empty matrix
  const int lds = (int)(sizeof(PairHead) + w_bytes + sizeof(unsigned) * BM_WORDS + sizeof(double) * PAIR_MAX_M);
  const long long items = std::max<long long>(1, (long long)p.P * ((p.P + 16 * WB - 1) / (16 * WB)));
  long long G = std::min<long long>(4LL * p.ncu, items);
  if (const char* e = getenv("MMSBM_PAIR_CENSUS_GRID")) {  // measurement: the number of workgroups
    const long long g = atoll(e);
    if (g >= 1) G = std::min<long long>(g, GRID_MAX);
  }

  DeviceGuard g(p.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  HIP_TRY(hipMemsetAsync(out_counts, 0, sizeof(int32_t) * (size_t)p.P * p.P * M, s));
  if (p.P < 3) return MMSBM_OK;
  scan_prep_kernel<<<dim3(p.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                  (double*)(w + p.off_T), p.K, p.KP, p.R, p.P, p.P16, s0);
  HIP_TRY(hipGetLastError());
  PairArgs a{};
  a.thT = (const double*)(w + p.off_thT);
  a.T = (const double*)(w + p.off_T);
  a.known = (const long long*)known;
  a.n_known = n_known;
  a.thresholds = thresholds;
  a.out = out_counts;
  a.K = p.K, a.P = p.P, a.P16 = p.P16, a.ns = ns, a.M = M, a.WB = WB;
  switch (p.KP / 4) {
    case 1: rc = launch_pair_census<1>(a, (int)G, lds, s); break;
    case 2: rc = launch_pair_census<2>(a, (int)G, lds, s); break;
    case 3: rc = launch_pair_census<3>(a, (int)G, lds, s); break;
    case 4: rc = launch_pair_census<4>(a, (int)G, lds, s); break;
    case 5: rc = launch_pair_census<5>(a, (int)G, lds, s); break;
    case 6: rc = launch_pair_census<6>(a, (int)G, lds, s); break;
    case 7: rc = launch_pair_census<7>(a, (int)G, lds, s); break;
    default: rc = launch_pair_census<8>(a, (int)G, lds, s); break;
  }
  return rc;
}

}  // extern "C"
