// pair_votes.hip — MI355X (gfx950) kernel + C ABI (include/mmsbm.h, mmsbm_pair_votes_*) of the pair
// vote census: for one threshold, M sorted vote levels and every pair of rank positions x < y, the
// exact number of eligible triples (the scan's: rank positions a < b < c < P, packed key not among
// the known ones) that contain both x and y and that at least levels[m] of the scored slots
// (restarts) score at or above the threshold.  The pair census counts on the ensemble mean; this
// call counts on agreement.
//
// Both halves exist.  The score phase, the per-slot compare and the hand-over of a tile with its
// votes packed one byte per element are the vote scan's (scan_sweep.h, sweep_votes and
// sweep_votes_masked; scan_score.h, Score<KS>::tile_votes), so a slot votes for a triple exactly when
// the vote scan says so and for every m the sum of out[x][y][m] over x < y is three times the tail
// of the vote scan's histogram from levels[m] on.  The binning is the pair census's
// (pair_census.hip), with `votes >= levels[t]` where it tests `score >= thresholds[t]`:
//   one ballot on "an eligible element with votes >= levels[0]" ends nearly every tile;
//   a tile with hits walks the levels upwards and stops at the first without a hit in the tile (the
//   levels do not decrease, so the later ones have none either);
//   (a, b): the 16 lanes of one kk share a row: one ballot per row, one add per nonzero (row, level);
//   (a, c): a lane's four elements share column c: added in the lane, the four kk groups by two
//           cross-lane moves, one add per nonzero (column, level) from the lanes of kk = 0;
//   (b, c): one add per hit and level.
// Those 25 lines are written again here and not shared: pair_census.hip records what a small change
// of its structure cost in registers, and a copy leaves its four kernels what they were.
//
// The levels are kernel arguments.  A level lies in [1, ns] and ns below 256 (the votes travel one
// byte per element), so the M <= 8 levels are one 64-bit argument, level t in byte t: the walk
// shifts a scalar register.  They need no device copy, no LDS table and no indexed read of the
// argument block (which would put the block into scratch).
//
// Every add is an integer add: registers, ballots and integer cross-lane moves, and relaxed
// agent-scope 32-bit atomic adds into the output, which the call has zeroed.  No floating-point
// value crosses a lane, so the counts do not depend on the grid, the batch or the arrival order.

#include <hip/hip_runtime.h>

#include <cmath>
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

constexpr int PAIR_VOTES_MAX_M = 8;      // documented cap of M (include/mmsbm.h): one byte of `levels` each
constexpr int PAIR_VOTES_MAX_P = 16384;  // the pair census's cap: x P + y < 2^28, the output at most 8 GiB

struct PairVotesArgs : SweepArgs {
  double threshold;
  unsigned long long levels;  // byte t: levels[t] in [1, ns], non-decreasing; bytes from M on are 0
  int* out;                   // [P][P][M], zeroed; only x < y is touched
  int M;                      // in [1, 8]
};

// The masked entry (mmsbm_pair_votes_masked): the pair mask travels in the masked kernels' own
// argument struct, as the vote scan's does.
struct PairVotesMaskedArgs : PairVotesArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

__device__ __forceinline__ void add(int* p, int v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The body of both kernels; ENS: the ensemble (ns > 1; a single sample otherwise), the sweep's
// template parameter; MASK: Args is PairVotesMaskedArgs and row a of the mask lies behind the bitmap
// in LDS.  A blocked element has left el before the binning sees it, so the binning is one.
template <int KS, bool ENS, bool MASK, class Args>
__device__ __forceinline__ void pair_votes_body(const Args& A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Head* st = reinterpret_cast<Head*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Head));
  unsigned* bm = reinterpret_cast<unsigned*>(W + (size_t)A.ns * 16 * A.WB * Score<KS>::WS);  // [BM_WORDS]

  sweep_begin(st);

  const int lane = threadIdx.x & 63, m = lane & 15, kk = lane >> 4;
  const int P = A.P, M = A.M;
  const unsigned long long levels = A.levels;
  const int lv0 = (int)(levels & 255u);  // M >= 1, lv0 >= 1
  int* const out = A.out;

  auto begin_item = [&](int a, int b0) {
    // once per item, not per tile with hits: the 64-bit product stays out of the binning
    const size_t rowa = (size_t)a * P;  // out[a][.][.]
    // Bin one finished tile's votes.
    return [&, rowa, b0](int ct, const d4v&, unsigned votes, const bool (&el)[4]) {
      // the eligible elements' votes, still one byte each (in [0, ns]); 0 for the others, which no
      // level (all >= 1) then counts
      const unsigned ev = votes & ((el[0] ? 0xffu : 0u) | (el[1] ? 0xff00u : 0u) | (el[2] ? 0xff0000u : 0u) |
                                   (el[3] ? 0xff000000u : 0u));
      // nearly every tile ends here when the threshold sits high in the distribution
      if (!__ballot((int)(ev & 255u) >= lv0 || (int)((ev >> 8) & 255u) >= lv0 || (int)((ev >> 16) & 255u) >= lv0 ||
                    (int)(ev >> 24) >= lv0))
        return;
      const int c = ct * 16 + m;
      unsigned long long rest = levels;  // wave-uniform: the level of this turn in its low byte
#pragma nounroll
      for (int t = 0; t < M; ++t, rest >>= 8) {
        const int lv = (int)(rest & 255u);
        unsigned long long hits = 0;  // the wave's hits at or above levels[t]
        int col = 0;                  // this lane's hits of column c at or above levels[t]
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const bool h = (int)((ev >> (8 * i)) & 255u) >= lv;  // only where el: a < b < c < P, every index in range
          col += (int)h;
          if (h) add(&out[((size_t)(b0 + kk + 4 * i) * P + c) * M + t], 1);  // (b, c)
          // (a, b): lanes 16 kk .. 16 kk + 15 of the ballot hold row b0 + kk + 4 i
          const unsigned long long mk = __ballot(h);
          hits |= mk;
          const int row = __popcll((mk >> (16 * kk)) & 0xffffull);
          if (m == 0 && row) add(&out[(rowa + (b0 + kk + 4 * i)) * M + t], row);  // row > 0 only where a < b < P
        }
        if (!hits) break;  // the levels do not decrease: no hit at the later ones either
        col += __shfl_xor(col, 16, 64);
        col += __shfl_xor(col, 32, 64);
        if (kk == 0 && col) add(&out[(rowa + c) * M + t], col);  // (a, c): col > 0 only where c < P
      }
    };
  };
  if constexpr (MASK)
    sweep_votes_masked<KS, ENS>(A, st, W, bm, A.threshold, A.mask, A.MW, bm + BM_WORDS, begin_item);
  else
    sweep_votes<KS, ENS>(A, st, W, bm, A.threshold, begin_item);
}

// The occupancy bounds start from those of the vote scan's histogram-only kernels (scan_votes.hip),
// for their reasons: at most 4 waves per SIMD, which sweep_grid's 4 workgroups per compute unit are
// sized for, and for the single sample 4 as the floor too.  The binning's addresses cost more
// registers than that kernel's LDS counters, so the floor ends one step earlier: under it the single
// sample of K = 29..32 spilled 3 VGPRs (16 bytes of scratch); under the cap alone it takes a 3-wave
// budget and no scratch (profiles/pair_votes_resources.txt).
template <int KS, bool ENS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(ENS || KS > 7 ? 1 : 4, 4))) void pair_votes_kernel(
    PairVotesArgs A) {
  pair_votes_body<KS, ENS, false>(A);
}

// The masked single sample keeps the floor of 4 waves up to K = 12 only (scan_votes_masked_kernel's
// histogram-only instantiation: up to K = 16; here K = 13..16 spilled 4 VGPRs under it): above, the
// mask's registers do not fit 128 VGPRs beside the operands.
template <int KS, bool ENS>
__global__ __launch_bounds__(NT)
    __attribute__((amdgpu_waves_per_eu(ENS || KS > 3 ? 1 : 4, 4))) void pair_votes_masked_kernel(
        PairVotesMaskedArgs A) {
  pair_votes_body<KS, ENS, true>(A);
}

struct PairVotesPlan {
  ScanShape sh;
  size_t off_thT, off_T, total;
};

// The workspace follows the context's shape only.
int make_plan(const mmsbm_ctx* c, PairVotesPlan* p) {
  if (int rc = scan_shape(c, "the pair vote census", &p->sh)) return rc;
  if (p->sh.P > PAIR_VOTES_MAX_P)
    return fail(MMSBM_ERR_UNSUPPORTED, "P=%d above the pair vote census's cap of %d (a P x P x M matrix)", p->sh.P,
                PAIR_VOTES_MAX_P);
  size_t off = 256;
  score_workspace(p->sh, off, &p->off_thT, &p->off_T);
  p->total = off;
  return MMSBM_OK;
}

// Both entry points; `masked`: mmsbm_pair_votes_masked, whose mask must not be null.
int pair_votes_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
                    bool masked, const double* theta, const double* pr, int32_t sample, double threshold,
                    const int32_t* levels_host, int32_t M, void* ws, int64_t ws_bytes, int32_t* out_counts,
                    void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  PairVotesPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  if (M < 0) return fail(MMSBM_ERR_INVALID, "M=%d < 0", M);
  if (M > PAIR_VOTES_MAX_M)
    return fail(MMSBM_ERR_UNSUPPORTED, "M=%d above the pair vote census's cap of %d", M, PAIR_VOTES_MAX_M);
  if (!order || !theta || !pr || (M > 0 && (!levels_host || !out_counts)))
    return fail(MMSBM_ERR_INVALID, "null pointer");
  if (!std::isfinite(threshold)) return fail(MMSBM_ERR_INVALID, "the threshold must be a finite number");
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "the pair vote census", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "the pair vote census", "mmsbm_pair_votes_workspace_bytes", known, n_known, sample, ws,
                       ws_bytes, p.total, &ns, &s0)))
    return rc;
  unsigned long long levels = 0;
  for (int t = 0; t < M; ++t) {
    const int lv = levels_host[t];
    if (lv < 1 || lv > ns)
      return fail(MMSBM_ERR_INVALID, "levels[%d]=%d outside [1, %d], the scored slots", t, lv, ns);
    if (t > 0 && lv < levels_host[t - 1])
      return fail(MMSBM_ERR_INVALID, "levels[%d]=%d below levels[%d]=%d: the levels must not decrease", t, lv, t - 1,
                  levels_host[t - 1]);
    levels |= (unsigned long long)lv << (8 * t);
  }
  if ((rc = pick_wb(sh, "the pair vote census", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  // a vote count is one byte of the sweep's hand-over and a level one byte of `levels`; the W tile's
  // 64 KiB holds far fewer slots than that (at most 85, K <= 4), so this never fires
  if (ns > 255) return fail(MMSBM_ERR_UNSUPPORTED, "the pair vote census: %d scored slots above 255", ns);
  if (M == 0) return MMSBM_OK;  // an empty matrix
  const int lds = (int)(sizeof(Head) + w_bytes + sizeof(unsigned) * (BM_WORDS + MW));
  const int G = sweep_grid(sh, WB, "MMSBM_PAIR_VOTES_GRID");

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  HIP_TRY(hipMemsetAsync(out_counts, 0, sizeof(int32_t) * (size_t)sh.P * sh.P * M, s));
  if (sh.P < 3) return MMSBM_OK;
  scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                   (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P, sh.P16, s0);
  HIP_TRY(hipGetLastError());
  const PairVotesArgs a{{(const double*)(w + p.off_thT), (const double*)(w + p.off_T), (const long long*)known,
                         n_known, sh.K, sh.P, sh.P16, ns, WB},
                        threshold, levels, out_counts, M};
  const PairVotesMaskedArgs am{a, mask, MW};
  return dispatch_ks(sh.KP / 4, [&](auto ks) {
    constexpr int KS = decltype(ks)::value;
    if (masked)
      return ns > 1 ? launch_lds(pair_votes_masked_kernel<KS, true>, G, lds, s, am)
                    : launch_lds(pair_votes_masked_kernel<KS, false>, G, lds, s, am);
    return ns > 1 ? launch_lds(pair_votes_kernel<KS, true>, G, lds, s, a)
                  : launch_lds(pair_votes_kernel<KS, false>, G, lds, s, a);
  });
}

}  // namespace

extern "C" {

int mmsbm_pair_votes_max_m(void) { return PAIR_VOTES_MAX_M; }

int mmsbm_pair_votes_workspace_bytes(const mmsbm_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  PairVotesPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_pair_votes(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const double* theta,
                     const double* pr, int32_t sample, double threshold, const int32_t* levels_host, int32_t M,
                     void* ws, int64_t ws_bytes, int32_t* out_counts, void* stream) {
  return pair_votes_call(c, order, known, n_known, nullptr, false, theta, pr, sample, threshold, levels_host, M, ws,
                         ws_bytes, out_counts, stream);
}

int mmsbm_pair_votes_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                            const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                            double threshold, const int32_t* levels_host, int32_t M, void* ws, int64_t ws_bytes,
                            int32_t* out_counts, void* stream) {
  return pair_votes_call(c, order, known, n_known, mask, true, theta, pr, sample, threshold, levels_host, M, ws,
                         ws_bytes, out_counts, stream);
}

}  // extern "C"
