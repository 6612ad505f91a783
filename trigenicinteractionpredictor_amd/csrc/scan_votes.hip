// scan_votes.hip — MI355X (gfx950) kernel + C ABI (include/mmsbm.h, mmsbm_scan_votes_*) of the vote
// scan: for every eligible triple (the scan's: rank positions a < b < c < P, packed key not among
// the known ones) the number of scored slots (restarts) whose own score is at or above one
// threshold, its votes; as a histogram over the votes, hist[0 .. ns], and as rows (votes, packed
// key, ensemble score) of the triples with at least min_votes of them.
//
// The score phase is the scan's, with one addition (scan_score.h, Score<KS>::tile_votes): the
// ensemble path has always formed each slot's 16 x 16 tile from zero before adding it to the
// slot-order sum; here the four elements of that accumulator are compared with the threshold first.
// The accumulator is the slot's single-sample score bit for bit (tile_one's MFMA chain over the same
// W row and Th' column), so a slot votes for a triple exactly when a census or a threshold scan of
// that slot alone counts it, and the mean that comes out is tile_mean's, bit for bit.  A single
// slot (ns = 1) keeps the register-resident single-sample path and compares its one tile.  The work
// items, the item skipping, the eligibility tests and the bitmap-guided known-key lookups are the
// sweep's (scan_sweep.h, sweep_votes), which hands over (tile, votes) one tile late as it hands
// over the tile elsewhere.
//
// Binning.  The workgroup holds ns + 1 counters in LDS.  One ballot decides whether a tile has an
// eligible triple with any vote at all; when it has none (with a threshold high in the
// distribution, nearly every tile) the wave adds the tile's eligible elements (four popcounts) to
// its private zero-vote count, as the census keeps `below`, and the tile is done.  Otherwise an
// element with votes adds 1 to the counter of its votes with an LDS atomic (when every such lane of
// the wave lands on one counter, one lane adds the wave's count instead).  At the workgroup's end
// the private counts join counter 0 and every nonzero counter goes to out_hist, which the call has
// zeroed, with one 64-bit global atomic add.
//
// Rows.  A hit is an eligible triple with votes >= min_votes.  Hits are compacted exactly as the
// threshold scan compacts its hits (scan_above.hip: one ballot per element, the wave's own staging
// buffer of STAGE rows in LDS, one relaxed agent-scope add on a 64-bit cursor per flush, the
// capacity guard on every row stored); a staged row carries the 4-byte vote count next to the score
// and the key.  A histogram-only call (capacity = 0) runs the instantiation without any of it and
// takes its count from the histogram.
//
// Everything that crosses a lane or a workgroup is an integer (ballots, popcounts, LDS and global
// integer adds, the cursor), and no floating-point value is combined beyond the score phase's own
// fixed-order sums: hist, the set of rows and every row's bits do not depend on the grid, the batch
// or the arrival order.  The order of the rows does.

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

// Every counter and the cursor count triples of one call: at most C(P, 3) < 2^63 (packed_keys_fit).
typedef unsigned long long count_t;

struct VotesArgs : SweepArgs {
  double threshold;
  int min_votes;        // in [1, ns]
  count_t capacity;     // rows of out_scores / out_keys / out_votes
  count_t* hist;        // [ns + 1], zeroed: hist[v] = eligible triples with v votes
  count_t* cursor;      // zeroed: the rows reserved so far
  double* out_scores;   // [capacity]
  long long* out_keys;  // [capacity]
  int* out_votes;       // [capacity]
};

// The masked vote scan (mmsbm_scan_votes_masked): the pair mask travels in the masked kernels' own
// argument struct, so VotesArgs and the unmasked kernels are what they were.
struct VotesMaskedArgs : VotesArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

constexpr int STAGE = 256;  // rows of a wave's staging buffer: the most one tile can hold
constexpr int ROW_BYTES = (int)(sizeof(double) + sizeof(long long) + sizeof(int));
constexpr int STAGE_BYTES = (NT / 64) * STAGE * ROW_BYTES;  // per workgroup: 20 KiB

// The body of both kernels; MASK: Args is VotesMaskedArgs and row a of the mask lies behind the
// bitmap, before the staging buffers (MW rounded up to 2 words, so that they stay 8-byte aligned).
template <int KS, bool ENS, bool LIST, bool MASK, class Args>
__device__ __forceinline__ void scan_votes_body(const Args& A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Head* st = reinterpret_cast<Head*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Head));
  const int ns = A.ns;
  count_t* cnt = reinterpret_cast<count_t*>(W + (size_t)ns * 16 * A.WB * Score<KS>::WS);  // [ns + 1]
  unsigned* bm = reinterpret_cast<unsigned*>(cnt + ns + 1);                                // [BM_WORDS]
  // this wave's staging buffer: [STAGE] scores, [STAGE] keys, then [STAGE] votes.  The offset from
  // smem is a multiple of 8: Head 64, W and cnt whole doublewords, the bitmap 1 KiB, a wave 5 KiB.
  int mrow_words = 0;
  if constexpr (MASK) mrow_words = (A.MW + 1) & ~1;
  char* stage =
      reinterpret_cast<char*>(bm + BM_WORDS + mrow_words) + (size_t)(threadIdx.x >> 6) * STAGE * ROW_BYTES;
  double* ssc = reinterpret_cast<double*>(stage);
  long long* sky = reinterpret_cast<long long*>(ssc + STAGE);
  int* svt = reinterpret_cast<int*>(sky + STAGE);

  for (int i = threadIdx.x; i <= ns; i += NT) cnt[i] = 0;
  sweep_begin(st);

  const int lane = threadIdx.x & 63, m = lane & 15, kk = lane >> 4;
  const int min_votes = A.min_votes;
  const count_t capacity = A.capacity;
  const int P = A.P;
  // this wave's eligible triples without a vote: popcounts of ballots, so wave-uniform (it lives in
  // scalar registers, where the census's per-lane `below` would take two vector registers here)
  count_t zero = 0;
  int fill = 0;      // rows staged by this wave (wave-uniform)

  // Reserve `fill` rows with one add and copy the staged rows out.  The whole wave calls it.
  auto flush = [&]() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // the staged rows, to the other lanes
    __builtin_amdgcn_wave_barrier();
    count_t base = 0;
    if (lane == 0) base = __hip_atomic_fetch_add(A.cursor, (count_t)fill, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    base = __shfl(base, 0, 64);
    for (int r = lane; r < fill; r += 64) {  // r < fill <= STAGE: inside the buffer
      const count_t row = base + (count_t)r;
      if (row < capacity) {  // the capacity guard: no address past the arrays is formed
        A.out_scores[row] = ssc[r];
        A.out_keys[row] = sky[r];
        A.out_votes[row] = svt[r];
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // read before the next tile overwrites it
    __builtin_amdgcn_wave_barrier();
    fill = 0;
  };

  auto begin_item = [&](int a, int b0) {
    // once per item: the key of (a, b0, column 0), the same for the whole wave.  A lane adds its
    // (kk + 4 i) P + c < 16 P + P16 <= 3.4 10^7 (packed_keys_fit: P <= 2 10^6) in 32 bits.
    // b0 comes from the wave's index, which the compiler takes for a vector value: read back through
    // lane 0, the key lives in scalar registers (with it in two vector registers the K > 28 single
    // sample spilled two).
    const long long key0w = ((long long)a * P + b0) * P;
    const long long key0 = ((long long)__builtin_amdgcn_readfirstlane((int)(key0w >> 32)) << 32) |
                           (unsigned)__builtin_amdgcn_readfirstlane((int)key0w);
    // Bin one finished tile's votes and stage its hits.
    return [&, key0](int ct, const d4v& tot, unsigned votes, const bool (&el)[4]) {
      // the eligible elements' votes, still one byte each (in [0, ns]); 0 for the others
      const unsigned ev = votes & ((el[0] ? 0xffu : 0u) | (el[1] ? 0xff00u : 0u) | (el[2] ? 0xff0000u : 0u) |
                                   (el[3] ? 0xff000000u : 0u));
      // nearly every tile ends here when the threshold sits high in the distribution
      if (!__ballot(ev != 0)) {
        zero += (count_t)(__popcll(__ballot(el[0])) + __popcll(__ballot(el[1])) + __popcll(__ballot(el[2])) +
                          __popcll(__ballot(el[3])));
        return;
      }
      // Rows first, so that the scores are dead before the counters are (fewer live registers).
      unsigned long long mk[4];
      int n = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // min_votes >= 1: never an ineligible element
        mk[i] = __ballot((int)((ev >> (8 * i)) & 255u) >= min_votes);
        n += __popcll(mk[i]);
      }
      if (LIST && n) {                  // wave-uniform
        if (fill + n > STAGE) flush();  // wave-uniform; n <= 256 = STAGE fits an empty buffer
        const int kc = kk * P + ct * 16 + m;  // element i: + 4 i P
        int at = fill;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // + the hits of element i in the lanes below this one: r < fill + n <= STAGE
          const int r = at + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk[i] >> 32),
                                                            __builtin_amdgcn_mbcnt_lo((unsigned)mk[i], 0u));
          const int v = (int)((ev >> (8 * i)) & 255u);
          if (v >= min_votes) {
            ssc[r] = tot[i];
            sky[r] = key0 + (kc + 4 * i * P);
            svt[r] = v;
          }
          at += __popcll(mk[i]);
        }
        fill += n;
      }
      // Counters: an element with votes adds 1 to the counter of its votes.
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = (int)((ev >> (8 * i)) & 255u);
        const bool in = v > 0;  // v <= ns: inside the counters
        zero += (count_t)__popcll(__ballot(el[i] && !in));
        const unsigned long long inm = __ballot(in);
        if (!inm) continue;
        const int first = __shfl(v, __ffsll((long long)inm) - 1, 64);
        if (!__ballot(in && v != first)) {  // one counter for the whole wave: one add
          if (lane == 0) atomicAdd(&cnt[first], (count_t)__popcll(inm));
        } else if (in) {
          atomicAdd(&cnt[v], (count_t)1);
        }
      }
    };
  };
  if constexpr (MASK)
    sweep_votes_masked<KS, ENS>(A, st, W, bm, A.threshold, A.mask, A.MW, bm + BM_WORDS, begin_item);
  else
    sweep_votes<KS, ENS>(A, st, W, bm, A.threshold, begin_item);
  if (LIST && fill) flush();  // wave-uniform
  if (zero && lane == 0) atomicAdd(&cnt[0], zero);
  __syncthreads();
  for (int i = threadIdx.x; i <= ns; i += NT) {
    const count_t c = cnt[i];
    if (c) __hip_atomic_fetch_add(&A.hist[i], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// The occupancy bounds are the threshold scan's (scan_above.hip), for its reasons: at most 4 waves
// per SIMD, which sweep_grid's 4 workgroups per compute unit are sized for, and for the single
// sample 4 as the floor too.  LIST: the call has rows to write (capacity > 0).  The histogram-only
// call is the instantiation without the staging, which holds 11 to 35 registers fewer (the ensemble
// of K = 13..16 and 25..28 then keeps 4 waves per SIMD where the listing kernel keeps 3).
template <int KS, bool ENS, bool LIST>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(ENS ? 1 : 4, 4))) void scan_votes_kernel(
    VotesArgs A) {
  scan_votes_body<KS, ENS, LIST, false>(A);
}

// The masked single sample keeps the floor of 4 waves up to K = 16 only (the listing kernel, which
// spilled one VGPR under it at K = 13..16: up to K = 12), as scan_above_masked_kernel does and for its
// reason: above, the mask's registers do not fit 128 VGPRs beside the operands and
// the floor would spill them; under the cap alone those kernels take a 3-wave budget and no scratch
// (profiles/scan_masked_families_resources.txt).
template <int KS, bool ENS, bool LIST>
__global__ __launch_bounds__(NT)
    __attribute__((amdgpu_waves_per_eu(ENS || KS > (LIST ? 3 : 4) ? 1 : 4, 4))) void scan_votes_masked_kernel(
        VotesMaskedArgs A) {
  scan_votes_body<KS, ENS, LIST, true>(A);
}

// The number of hits: the cursor of a listing call; a histogram-only call reserved no row, and its
// count is the histogram's, hist[min_votes .. ns] added up (the two agree: a hit is staged exactly
// when it is binned at or above min_votes).
__global__ void scan_votes_finish_kernel(const count_t* __restrict__ cursor, const count_t* __restrict__ hist,
                                         int ns, int min_votes, bool listed, long long* __restrict__ out_count) {
  count_t n = 0;
  if (listed) {
    n = *cursor;
  } else {
    for (int v = min_votes; v <= ns; ++v) n += hist[v];
  }
  *out_count = (long long)n;
}

struct VotesPlan {
  ScanShape sh;
  size_t off_thT, off_T, off_cursor, total;
};

// The workspace follows the context's shape only.
int make_plan(const mmsbm_ctx* c, VotesPlan* p) {
  if (int rc = scan_shape(c, "the vote scan", &p->sh)) return rc;
  if (int rc = packed_keys_fit(p->sh)) return rc;
  size_t off = 256;
  score_workspace(p->sh, off, &p->off_thT, &p->off_T);
  p->off_cursor = off, off = align256(off + sizeof(count_t));
  p->total = off;
  return MMSBM_OK;
}

// Both entry points; `masked`: mmsbm_scan_votes_masked, whose mask must not be null.
int votes_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
               bool masked, const double* theta, const double* pr, int32_t sample, double threshold,
               int32_t min_votes, int64_t capacity, void* ws, int64_t ws_bytes, int64_t* out_hist,
               double* out_scores, int64_t* out_keys, int32_t* out_votes, int64_t* out_count, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  VotesPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  if (!order || !theta || !pr || !out_hist || !out_count) return fail(MMSBM_ERR_INVALID, "null pointer");
  if (!std::isfinite(threshold)) return fail(MMSBM_ERR_INVALID, "the threshold must be a finite number");
  if (capacity < 0) return fail(MMSBM_ERR_INVALID, "capacity=%lld < 0", (long long)capacity);
  if (capacity > 0 && (!out_scores || !out_keys || !out_votes))
    return fail(MMSBM_ERR_INVALID, "null output array with capacity > 0");
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "the vote scan", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "the vote scan", "mmsbm_scan_votes_workspace_bytes", known, n_known, sample, ws, ws_bytes,
                       p.total, &ns, &s0)))
    return rc;
  if (min_votes < 1 || min_votes > ns)
    return fail(MMSBM_ERR_INVALID, "min_votes=%d outside [1, %d], the scored slots", min_votes, ns);
  if ((rc = pick_wb(sh, "the vote scan", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  const int mrow_words = (MW + 1) & ~1;  // the masked kernel's mask row, before the staging buffers
  const int lds =
      (int)(sizeof(Head) + w_bytes + sizeof(count_t) * (ns + 1) + sizeof(unsigned) * (BM_WORDS + mrow_words)) +
      (capacity > 0 ? STAGE_BYTES : 0);  // a histogram-only call stages nothing
  const int G = sweep_grid(sh, WB, "MMSBM_SCAN_VOTES_GRID");

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  count_t* cursor = (count_t*)(w + p.off_cursor);
  HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(count_t), s));
  HIP_TRY(hipMemsetAsync(out_hist, 0, sizeof(count_t) * ((size_t)ns + 1), s));
  if (sh.P >= 3) {
    scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                     (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P, sh.P16, s0);
    HIP_TRY(hipGetLastError());
    const VotesArgs a{{(const double*)(w + p.off_thT), (const double*)(w + p.off_T), (const long long*)known,
                       n_known, sh.K, sh.P, sh.P16, ns, WB},
                      threshold, min_votes, (count_t)capacity, (count_t*)out_hist, cursor, out_scores,
                      (long long*)out_keys, out_votes};
    const VotesMaskedArgs am{a, mask, MW};
    rc = dispatch_ks(sh.KP / 4, [&](auto ks) {
      constexpr int KS = decltype(ks)::value;
      if (masked) {
        if (capacity > 0)
          return ns > 1 ? launch_lds(scan_votes_masked_kernel<KS, true, true>, G, lds, s, am)
                        : launch_lds(scan_votes_masked_kernel<KS, false, true>, G, lds, s, am);
        return ns > 1 ? launch_lds(scan_votes_masked_kernel<KS, true, false>, G, lds, s, am)
                      : launch_lds(scan_votes_masked_kernel<KS, false, false>, G, lds, s, am);
      }
      if (capacity > 0)
        return ns > 1 ? launch_lds(scan_votes_kernel<KS, true, true>, G, lds, s, a)
                      : launch_lds(scan_votes_kernel<KS, false, true>, G, lds, s, a);
      return ns > 1 ? launch_lds(scan_votes_kernel<KS, true, false>, G, lds, s, a)
                    : launch_lds(scan_votes_kernel<KS, false, false>, G, lds, s, a);
    });
    if (rc) return rc;
  }
  scan_votes_finish_kernel<<<1, 1, 0, s>>>(cursor, (const count_t*)out_hist, ns, min_votes, capacity > 0,
                                           (long long*)out_count);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

}  // namespace

extern "C" {

int mmsbm_scan_votes_workspace_bytes(const mmsbm_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  VotesPlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_scan_votes(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                     const double* theta, const double* pr, int32_t sample, double threshold, int32_t min_votes,
                     int64_t capacity, void* ws, int64_t ws_bytes, int64_t* out_hist, double* out_scores,
                     int64_t* out_keys, int32_t* out_votes, int64_t* out_count, void* stream) {
  return votes_call(c, order, known, n_known, nullptr, false, theta, pr, sample, threshold, min_votes, capacity, ws,
                    ws_bytes, out_hist, out_scores, out_keys, out_votes, out_count, stream);
}

int mmsbm_scan_votes_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                            const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                            double threshold, int32_t min_votes, int64_t capacity, void* ws, int64_t ws_bytes,
                            int64_t* out_hist, double* out_scores, int64_t* out_keys, int32_t* out_votes,
                            int64_t* out_count, void* stream) {
  return votes_call(c, order, known, n_known, mask, true, theta, pr, sample, threshold, min_votes, capacity, ws,
                    ws_bytes, out_hist, out_scores, out_keys, out_votes, out_count, stream);
}

}  // extern "C"
