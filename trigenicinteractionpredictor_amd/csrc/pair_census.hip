// pair_census.hip — MI355X (gfx950) kernel + C ABI (include/mmsbm.h, mmsbm_pair_census_*) of the
// pair census: for M sorted thresholds and every pair of rank positions x < y, the exact number of
// eligible triples (the scan's: rank positions a < b < c < P, packed key not among the known ones)
// that contain both x and y and whose score is at or above each threshold.
//
// The score phase is the scan's (scan_score.h: the same prep, W rows, MFMA chain per tile and, for
// the ensemble, the same slot-order sum and division); the work items, the item skipping, the
// eligibility tests and the bitmap-guided known-key lookups are the sweep's (scan_sweep.h), which
// the census (census.hip) runs too, so the same triples are hits here and there: for every m, the
// sum of out[x][y][m] over x < y is three times the census count at thresholds[m], exactly.
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

constexpr int PAIR_MAX_M = 8;       // documented cap of M (include/mmsbm.h)
constexpr int PAIR_MAX_P = 16384;   // documented cap of P: x P + y < 2^28, the output at most 8 GiB

// Flat, in this order, and the kernel hands the sweep its fields: with a SweepArgs inside (as a
// base or a member, in any place tried) the kernel spills more scalar registers, 1 % at K = 10, B = 8.
struct PairArgs {
  const double* thT;        // [ns][KP][P16]
  const double* T;          // [ns][P][K][KP]
  const long long* known;   // sorted packed keys (null: none)
  long long n_known;
  const double* thresholds; // [M], non-decreasing, M >= 1
  int* out;                 // [P][P][M], zeroed; only x < y is touched
  int K, P, P16, ns, M, WB;
};

// The masked pair census (mmsbm_pair_census_masked): the pair mask travels in the masked kernels' own
// argument struct, flat as PairArgs is, so PairArgs and the unmasked kernels are what they were.
struct PairMaskedArgs {
  const double* thT;
  const double* T;
  const long long* known;
  long long n_known;
  const double* thresholds;
  int* out;
  const unsigned* mask;     // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int K, P, P16, ns, M, WB, MW;
};

__device__ __forceinline__ void add(int* p, int v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// ENS: the ensemble (ns > 1; a single sample otherwise), the sweep's template parameter.  It is one
// so that neither path holds the other's registers: one kernel for both took 132 VGPRs at
// K = 10 against the census's 120, which leaves 3 workgroups per CU of the 4 the grid is sized for;
// split, the single-sample kernel takes 108 and the ensemble's 120.
// The body of both kernels; MASK: Args is PairMaskedArgs and row a of the mask lies behind the
// thresholds in LDS.  A blocked element has left el before the binning sees it, so the binning is one.
template <int KS, bool ENS, bool MASK, class Args>
__device__ __forceinline__ void pair_census_body(const Args& A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Head* st = reinterpret_cast<Head*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Head));
  const SweepArgs S{A.thT, A.T, A.known, A.n_known, A.K, A.P, A.P16, A.ns, A.WB};
  const int P = A.P, M = A.M;
  unsigned* bm = reinterpret_cast<unsigned*>(W + (size_t)A.ns * 16 * A.WB * Score<KS>::WS);  // [BM_WORDS]
  double* thr = reinterpret_cast<double*>(bm + BM_WORDS);                                   // [M]

  if (threadIdx.x < M) thr[threadIdx.x] = A.thresholds[threadIdx.x];
  sweep_begin(st);

  const int lane = threadIdx.x & 63, m = lane & 15, kk = lane >> 4;
  const double thr0 = A.thresholds[0];  // M >= 1
  int* const out = A.out;

  auto begin_item = [&](int a, int b0) {
    // once per item, not per tile with hits: the 64-bit product stays out of the binning
    const size_t rowa = (size_t)a * P;  // out[a][.][.]
    // Bin one finished tile.
    return [&, rowa, b0](int ct, const d4v& tot, const bool (&el)[4]) {
      // nearly every tile ends here when the thresholds sit high in the distribution
      if (!__ballot((el[0] && tot[0] >= thr0) || (el[1] && tot[1] >= thr0) || (el[2] && tot[2] >= thr0) ||
                    (el[3] && tot[3] >= thr0)))
        return;
      const int c = ct * 16 + m;
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
  };
  if constexpr (MASK)
    sweep_masked<KS, ENS>(S, st, W, bm, A.mask, A.MW, reinterpret_cast<unsigned*>(thr + PAIR_MAX_M), begin_item);
  else
    sweep<KS, ENS>(S, st, W, bm, begin_item);
}

template <int KS, bool ENS>
__global__ __launch_bounds__(NT) void pair_census_kernel(PairArgs A) {
  pair_census_body<KS, ENS, false>(A);
}

template <int KS, bool ENS>
__global__ __launch_bounds__(NT) void pair_census_masked_kernel(PairMaskedArgs A) {
  pair_census_body<KS, ENS, true>(A);
}

struct PairPlan {
  ScanShape sh;
  size_t off_thT, off_T, total;
};

// The workspace follows the context's shape only (M is checked here and needs no scratch).
int make_plan(const mmsbm_ctx* c, int M, PairPlan* p) {
  if (int rc = scan_shape(c, "pair census", &p->sh)) return rc;
  if (M < 0) return fail(MMSBM_ERR_INVALID, "M=%d < 0", M);
  if (M > PAIR_MAX_M) return fail(MMSBM_ERR_UNSUPPORTED, "M=%d above the pair census's cap of %d", M, PAIR_MAX_M);
  if (p->sh.P > PAIR_MAX_P)
    return fail(MMSBM_ERR_UNSUPPORTED, "P=%d above the pair census's cap of %d (a P x P x M matrix)", p->sh.P,
                PAIR_MAX_P);
  size_t off = 256;
  score_workspace(p->sh, off, &p->off_thT, &p->off_T);
  p->total = off;
  return MMSBM_OK;
}

// Both entry points; `masked`: mmsbm_pair_census_masked, whose mask must not be null.
int pair_census_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
                     bool masked, const double* theta, const double* pr, int32_t sample, const double* thresholds,
                     int32_t M, void* ws, int64_t ws_bytes, int32_t* out_counts, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  PairPlan p;
  int rc = make_plan(c, M, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  if (!order || !theta || !pr || (M > 0 && (!thresholds || !out_counts)))
    return fail(MMSBM_ERR_INVALID, "null pointer");
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "pair census", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "pair census", "mmsbm_pair_census_workspace_bytes", known, n_known, sample, ws, ws_bytes,
                       p.total, &ns, &s0)))
    return rc;
  if ((rc = pick_wb(sh, "pair census", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  if (M == 0) return MMSBM_OK;  // an empty matrix
  const int lds = (int)(sizeof(Head) + w_bytes + sizeof(unsigned) * (BM_WORDS + MW) + sizeof(double) * PAIR_MAX_M);
  const int G = sweep_grid(sh, WB, "MMSBM_PAIR_CENSUS_GRID");

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  HIP_TRY(hipMemsetAsync(out_counts, 0, sizeof(int32_t) * (size_t)sh.P * sh.P * M, s));
  if (sh.P < 3) return MMSBM_OK;
  scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                   (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P, sh.P16, s0);
  HIP_TRY(hipGetLastError());
  const PairArgs a{(const double*)(w + p.off_thT), (const double*)(w + p.off_T), (const long long*)known, n_known,
                   thresholds, out_counts, sh.K, sh.P, sh.P16, ns, M, WB};
  const PairMaskedArgs am{a.thT, a.T,  a.known, n_known, thresholds, out_counts, mask,
                          sh.K,  sh.P, sh.P16,  ns,      M,          WB,         MW};
  return dispatch_ks(sh.KP / 4, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    if (masked)
      return ns > 1 ? launch_lds(pair_census_masked_kernel<KS, true>, G, lds, s, am)
                    : launch_lds(pair_census_masked_kernel<KS, false>, G, lds, s, am);
    return ns > 1 ? launch_lds(pair_census_kernel<KS, true>, G, lds, s, a)
                  : launch_lds(pair_census_kernel<KS, false>, G, lds, s, a);
  });
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
  return pair_census_call(c, order, known, n_known, nullptr, false, theta, pr, sample, thresholds, M, ws, ws_bytes,
                          out_counts, stream);
}

int mmsbm_pair_census_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                             const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                             const double* thresholds, int32_t M, void* ws, int64_t ws_bytes, int32_t* out_counts,
                             void* stream) {
  return pair_census_call(c, order, known, n_known, mask, true, theta, pr, sample, thresholds, M, ws, ws_bytes,
                          out_counts, stream);
}

}  // extern "C"
