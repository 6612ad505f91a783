// scan_above.hip — MI355X (gfx950) kernel + C ABI (include/mmsbm.h, mmsbm_scan_above_*) of the
// threshold scan: every eligible triple (the scan's: rank positions a < b < c < P, packed key not
// among the known ones) whose score is at or above one threshold, as rows (score, packed key), and
// their number.
//
// The score phase is the scan's (scan_score.h: the same prep, W rows, MFMA chain per tile and, for
// the ensemble, the same slot-order sum and division); the work items, the item skipping, the
// eligibility tests and the bitmap-guided known-key lookups are the sweep's (scan_sweep.h), which
// the census (census.hip) runs too, so the same triples are hits here and there with the same score
// bits: the count returned here is the census's count at that threshold, exactly.
//
// Compaction.  A hit is an eligible triple with score >= threshold.  One ballot decides whether a
// tile has a hit; when it has none (with a threshold high in the distribution, nearly every tile)
// the tile is done.  In a tile with hits the wave takes one ballot per accumulator element and adds
// the four popcounts: its row count n.  A lane's hit i goes to slot fill + (hits of elements below
// i) + (hits of element i in lower lanes) of the wave's own staging buffer in LDS (STAGE rows of
// score and key; no other wave touches it, so no workgroup barrier is involved).
//
// Flush.  When a tile's n rows do not fit behind the `fill` rows staged, and once after the sweep,
// the wave flushes: one lane reserves `fill` rows with one relaxed agent-scope add on a 64-bit
// cursor in the workspace, which the call has zeroed; the base goes to the whole wave and lane l
// copies staged rows l, l + 64, ... to rows base + l, ... of the two output arrays, in 512-byte
// runs.  A lane stores only to rows below `capacity`: that one test guards every address formed
// from the cursor, which itself goes on counting, so the count is the full one whatever the
// capacity.  A tile has at most 256 = STAGE rows, so a tile of an empty buffer always fits.
// (One add per tile with hits, the first form, made every such tile wait for one address: at
// P = 1500 and 1 % hits, where nine tiles in ten hold a hit or two, 2 million adds took 10 ms.)
//
// Nothing but the integer cursor crosses a workgroup, within one only hits move (unchanged, through
// the wave's buffer), and no floating-point value is combined anywhere: the set of rows and each
// row's bits do not depend on the grid, the batch or the arrival order.  The order of the rows
// does: it follows the grid and the run.

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

// The cursor counts the hits of one call: at most C(P, 3) < 2^63 (packed_keys_fit), so it cannot wrap.
typedef unsigned long long count_t;

struct AboveArgs : SweepArgs {
  double threshold;
  count_t capacity;     // rows of out_scores / out_keys
  count_t* cursor;      // zeroed: the rows reserved so far
  double* out_scores;   // [capacity]
  long long* out_keys;  // [capacity]
};

// The masked threshold scan (mmsbm_scan_above_masked): the pair mask travels in the masked kernels'
// own argument struct, so AboveArgs and the unmasked kernels are what they were.
struct AboveMaskedArgs : AboveArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

constexpr int STAGE = 256;  // rows of a wave's staging buffer: the most one tile can hold
constexpr int STAGE_BYTES = (NT / 64) * STAGE * (int)(sizeof(double) + sizeof(long long));  // per workgroup

// At most 4 waves per SIMD: the census's cap (census.hip), which sweep_grid's 4 workgroups per
// compute unit are sized for.  For the single sample 4 is also the floor: with the cap alone the
// kernels of K > 24 took 121 and 126 VGPRs next to 8 AGPRs (spilled scalars), a 3-wave budget, and
// the K = 30 call with no hit ran at 2.96 ms against the census's 2.00 ms (P = 1500); with the
// floor they take 1.98 ms and no instantiation spills a VGPR or takes scratch.  The ensemble keeps
// the cap alone: under the floor its K = 10, B = 8 call with no hit ran at 6.98 ms against 5.51 ms.
// The body of both kernels; MASK: Args is AboveMaskedArgs and row a of the mask lies behind the
// staging buffers.
template <int KS, bool ENS, bool MASK, class Args>
__device__ __forceinline__ void scan_above_body(const Args& A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Head* st = reinterpret_cast<Head*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Head));
  unsigned* bm = reinterpret_cast<unsigned*>(W + (size_t)A.ns * 16 * A.WB * Score<KS>::WS);  // [BM_WORDS]
  // this wave's staging buffer: [STAGE] scores, then [STAGE] keys
  double* ssc = reinterpret_cast<double*>(bm + BM_WORDS) + (size_t)(threadIdx.x >> 6) * 2 * STAGE;
  long long* sky = reinterpret_cast<long long*>(ssc + STAGE);

  sweep_begin(st);

  const int lane = threadIdx.x & 63, m = lane & 15, kk = lane >> 4;
  const double thr = A.threshold;
  const count_t capacity = A.capacity;
  const int P = A.P;
  int fill = 0;  // rows staged by this wave (wave-uniform)

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
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // read before the next tile overwrites it
    __builtin_amdgcn_wave_barrier();
    fill = 0;
  };

  auto begin_item = [&](int a, int b0) {
    // once per item: the key of (a, b0, column 0), the same for the whole wave.  A lane adds its
    // (kk + 4 i) P + c < 16 P + P16 <= 3.4 10^7 (packed_keys_fit: P <= 2 10^6) in 32 bits.
    const long long key0 = ((long long)a * P + b0) * P;
    // Stage one finished tile's hits.
    return [&, key0](int ct, const d4v& tot, const bool (&el)[4]) {
      bool h[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) h[i] = el[i] && tot[i] >= thr;
      // nearly every tile ends here when the threshold sits high in the distribution
      if (!__ballot(h[0] || h[1] || h[2] || h[3])) return;
      unsigned long long mk[4];
      int n = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        mk[i] = __ballot(h[i]);
        n += __popcll(mk[i]);
      }
      if (fill + n > STAGE) flush();  // wave-uniform; n <= 256 = STAGE fits an empty buffer
      const int kc = kk * P + ct * 16 + m;  // element i: + 4 i P
      int at = fill;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // + the hits of element i in the lanes below this one: r < fill + n <= STAGE
        const int r = at + (int)__builtin_amdgcn_mbcnt_hi((unsigned)(mk[i] >> 32),
                                                          __builtin_amdgcn_mbcnt_lo((unsigned)mk[i], 0u));
        if (h[i]) {
          ssc[r] = tot[i];
          sky[r] = key0 + (kc + 4 * i * P);
        }
        at += __popcll(mk[i]);
      }
      fill += n;
    };
  };
  if constexpr (MASK)
    sweep_masked<KS, ENS>(A, st, W, bm, A.mask, A.MW,
                          reinterpret_cast<unsigned*>(reinterpret_cast<char*>(bm + BM_WORDS) + STAGE_BYTES), begin_item);
  else
    sweep<KS, ENS>(A, st, W, bm, begin_item);
  if (fill) flush();  // wave-uniform
}

template <int KS, bool ENS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(ENS ? 1 : 4, 4))) void scan_above_kernel(
    AboveArgs A) {
  scan_above_body<KS, ENS, false>(A);
}

// The masked single sample keeps the floor of 4 waves up to K = 16 only: above, the mask's registers
// (the four (b, c) halfwords in flight, the blocked bits of two tiles, the bases of the four rows) do
// not fit 128 VGPRs beside the operands and the floor would spill them to scratch; under the cap
// alone those kernels take a 3-wave budget and no scratch.
template <int KS, bool ENS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(ENS || KS > 4 ? 1 : 4, 4))) void scan_above_masked_kernel(
    AboveMaskedArgs A) {
  scan_above_body<KS, ENS, true>(A);
}

__global__ void scan_above_finish_kernel(const count_t* __restrict__ cursor, long long* __restrict__ out_count) {
  *out_count = (long long)*cursor;
}

struct AbovePlan {
  ScanShape sh;
  size_t off_thT, off_T, off_cursor, total;
};

// The workspace follows the context's shape only.
int make_plan(const mmsbm_ctx* c, AbovePlan* p) {
  if (int rc = scan_shape(c, "the threshold scan", &p->sh)) return rc;
  if (int rc = packed_keys_fit(p->sh)) return rc;
  size_t off = 256;
  score_workspace(p->sh, off, &p->off_thT, &p->off_T);
  p->off_cursor = off, off = align256(off + sizeof(count_t));
  p->total = off;
  return MMSBM_OK;
}

// Both entry points; `masked`: mmsbm_scan_above_masked, whose mask must not be null.
int above_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
               bool masked, const double* theta, const double* pr, int32_t sample, double threshold, int64_t capacity,
               void* ws, int64_t ws_bytes, double* out_scores, int64_t* out_keys, int64_t* out_count, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  AbovePlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  if (!order || !theta || !pr || !out_count) return fail(MMSBM_ERR_INVALID, "null pointer");
  if (!std::isfinite(threshold)) return fail(MMSBM_ERR_INVALID, "the threshold must be a finite number");
  if (capacity < 0) return fail(MMSBM_ERR_INVALID, "capacity=%lld < 0", (long long)capacity);
  if (capacity > 0 && (!out_scores || !out_keys))
    return fail(MMSBM_ERR_INVALID, "null output array with capacity > 0");
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "the threshold scan", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "the threshold scan", "mmsbm_scan_above_workspace_bytes", known, n_known, sample, ws,
                       ws_bytes, p.total, &ns, &s0)))
    return rc;
  if ((rc = pick_wb(sh, "the threshold scan", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  const int lds = (int)(sizeof(Head) + w_bytes + sizeof(unsigned) * (BM_WORDS + MW)) + STAGE_BYTES;
  const int G = sweep_grid(sh, WB, "MMSBM_SCAN_ABOVE_GRID");

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  count_t* cursor = (count_t*)(w + p.off_cursor);
  HIP_TRY(hipMemsetAsync(cursor, 0, sizeof(count_t), s));
  if (sh.P >= 3) {
    scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                     (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P, sh.P16, s0);
    HIP_TRY(hipGetLastError());
    const AboveArgs a{{(const double*)(w + p.off_thT), (const double*)(w + p.off_T), (const long long*)known,
                       n_known, sh.K, sh.P, sh.P16, ns, WB},
                      threshold, (count_t)capacity, cursor, out_scores, (long long*)out_keys};
    const AboveMaskedArgs am{a, mask, MW};
    rc = dispatch_ks(sh.KP / 4, [&](auto ks) {
      constexpr int KS = decltype(ks)::value;
      if (masked)
        return ns > 1 ? launch_lds(scan_above_masked_kernel<KS, true>, G, lds, s, am)
                      : launch_lds(scan_above_masked_kernel<KS, false>, G, lds, s, am);
      return ns > 1 ? launch_lds(scan_above_kernel<KS, true>, G, lds, s, a)
                    : launch_lds(scan_above_kernel<KS, false>, G, lds, s, a);
    });
    if (rc) return rc;
  }
  scan_above_finish_kernel<<<1, 1, 0, s>>>(cursor, (long long*)out_count);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

}  // namespace

extern "C" {

int mmsbm_scan_above_workspace_bytes(const mmsbm_ctx* c, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  AbovePlan p;
  int rc = make_plan(c, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_scan_above(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                     const double* theta, const double* pr, int32_t sample, double threshold,
                     int64_t capacity, void* ws, int64_t ws_bytes, double* out_scores, int64_t* out_keys,
                     int64_t* out_count, void* stream) {
  return above_call(c, order, known, n_known, nullptr, false, theta, pr, sample, threshold, capacity, ws, ws_bytes,
                    out_scores, out_keys, out_count, stream);
}

int mmsbm_scan_above_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                            const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                            double threshold, int64_t capacity, void* ws, int64_t ws_bytes, double* out_scores,
                            int64_t* out_keys, int64_t* out_count, void* stream) {
  return above_call(c, order, known, n_known, mask, true, theta, pr, sample, threshold, capacity, ws, ws_bytes,
                    out_scores, out_keys, out_count, stream);
}

}  // extern "C"
