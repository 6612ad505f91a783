// scan_spread.hip — MI355X (gfx950) kernels + C ABI (include/mmsbm.h, mmsbm_scan_spread_*) of the
// dispute scan: the exact top N of the spread d_t over the scan's eligible triples (rank positions
// a < b < c < P, packed key not among the known ones), d_t = q_{1+t} - q_{ns-t} with q_m the m-th
// largest of the scored slots' (restarts') own scores, as the quorum scan forms it.  t = 0 ranks by
// the range max - min; t = 1 drops the single highest and the single lowest restart, so that one
// stray restart cannot create a dispute; t = ns / 2 - 1 on an even ns is the gap between the two
// middle scores.  The list names the triples on which the restarts disagree most.
//
// The kernel is scan_quorum.hip's ensemble kernel with another score phase: the same work items (a,
// a block of 16 WB rows b) round-robin over the workgroups, the W rows of every slot in LDS, the
// same candidate buffer (LDS when it fits, else workspace), wave_reserve / wg_keep_best, the
// published bound, the seeding pass over every 61st item at P >= 200 and the fan-in-32 merge
// (scan_select.h, used as it is; the plan, the merge kernel and the host loop over the passes are
// scan_topn.h, shared with scan.hip and scan_quorum.hip; the kernel is restated here, so that
// scan.hip's and scan_quorum.hip's instantiations stay the objects they were).  Only the tile
// differs (scan_score.h, Score<KS>::tile_spread<D>, D = t + 1): each slot's 16 x 16 tile is formed
// from zero with the single-sample MFMA chain, as tile_mean forms it, and inserted into two
// per-element sorted lists of depth D in registers, the D largest and the D smallest.  d_t is one
// IEEE subtraction of two of the slots' scores; nothing else is combined across slots.  d_t >= +0,
// so the integer atomic max of the published bound orders it as it orders the scan's scores.
//
// No early exit.  The quorum scan leaves a tile's slot loop once no element can still reach the
// pruning bound, because q_m has an upper bound that falls as slots arrive.  A spread has none:
// top[D - 1] only rises and bot[D - 1] only falls with every further slot, so the spread of the
// slots seen so far is a lower bound of d_t, never an upper one, and any slot still to come can
// lift any element over the cut.  Every slot of every tile is formed; the cut prunes only after the
// slot loop, as in scan_kernel.
//
// There is no single-slot path: one restart has no spread, and the call refuses it.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mmsbm.h"
#include "scan_host.h"
#include "scan_score.h"
#include "scan_select.h"
#include "scan_topn.h"

namespace {

using namespace scan_host;
using namespace scan_select;
using namespace scan_topn;
using scan_score::Score;
using scan_score::W_LDS_MAX;

constexpr int SPREAD_MAX_TRIM = 3;   // two sorted lists of depth 4, the quorum scan's depth

struct SpreadArgs {
  const double* thT;          // [ns][KP][P16]
  const double* T;            // [ns][P][K][KP]
  const long long* known;     // sorted packed keys (null: none)
  long long n_known;
  double* cand_s;             // workspace candidate buffers [G][cap] (null: LDS)
  long long* cand_k;
  double* list_s;             // per-workgroup results [G][N]
  long long* list_k;
  int* list_n;                // [G]
  unsigned long long* shared; // published threshold bits
  int K, P, P16, ns, N, cap, WB;
  int stride;                 // 1: every item; > 1: the seeding pass over every stride-th item
};

// D = trim + 1 >= 1: the depth of the two sorted lists; ns >= 2 D (the host checks it).
template <int KS, int D>
__global__ __launch_bounds__(NT) void scan_spread_kernel(SpreadArgs A) {
  using Sc = Score<KS>;
  constexpr int WS = Sc::WS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));
  const int RB = 16 * A.WB;
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns;
  double* lcs = W + (size_t)ns * RB * WS;  // the candidate buffer when it is in LDS
  long long* lck = reinterpret_cast<long long*>(lcs + A.cap);
  double* cs = lcs;
  long long* ck = lck;
  if (A.cand_s) {
    cs = A.cand_s + (size_t)blockIdx.x * A.cap;
    ck = A.cand_k + (size_t)blockIdx.x * A.cap;
  }
  auto keep_best = [&]() {
    if (A.cand_s) wg_keep_best(st, cs, ck, A.N, A.shared);
    else wg_keep_best(st, lcs, lck, A.N, A.shared);
  };
  if (threadIdx.x == 0) sel_init(st);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const long long PP = (long long)P;

  for (long long q = (long long)blockIdx.x * A.stride; q < PP * nbq; q += (long long)gridDim.x * A.stride) {
    const int a = (int)(q / nbq), bq = (int)(q % nbq);
    if (a >= P - 2 || bq * RB + RB - 1 <= a || bq * RB >= P - 1) continue;  // no a < b < c here
    __syncthreads();  // the previous item's W is read
    if (threadIdx.x == 0) {
      const unsigned long long g = __hip_atomic_load(A.shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st->gthr = g ? __longlong_as_double((long long)g) : neg_inf();
    }
    if (threadIdx.x == 64 && A.n_known > 0) {  // the known keys whose first gene is a
      st->klo = lower_bound(A.known, 0, A.n_known, (long long)a * PP * PP);
      st->khi = lower_bound(A.known, st->klo, A.n_known, (long long)(a + 1) * PP * PP);
    }
    Sc::fill_w(W, A.T, A.thT, a, bq, RB, ns, K, P, P16);
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1 && b0 + 15 > a;
    int ct = bq * A.WB + wc;
    while (ct < btile) ct += CW;  // every c of those tiles is below every b
    const long long klo = st->klo, khi = st->khi;
    for (;;) {
      // the thresholds change only when the workgroup sorts its buffer (behind a barrier)
      const double thr_s = st->thr_s, gthr = st->gthr;
      const long long thr_k = st->thr_k;
      const double cut = fmax(thr_s, gthr);
      if (wave_on) {
        for (; ct < nct; ct += CW) {
          const int c0 = ct * 16;
          const d4v tot = Sc::template tile_spread<D>(W, A.thT, ns, RB, P16, wb, c0, m, kk);
          // lane holds d[b0 + kk + 4 i][c0 + m]; from here on scan_kernel's selection
          if (!__ballot(tot[0] >= cut || tot[1] >= cut || tot[2] >= cut || tot[3] >= cut)) continue;
          const int c = c0 + m;
          bool pass[4];
          long long key[4];
          unsigned long long mk[4];
          int n = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + kk + 4 * i;
            key[i] = ((long long)a * PP + b) * PP + c;
            pass[i] = a < b && b < c && c < P && !(tot[i] < gthr) && before(tot[i], key[i], thr_s, thr_k);
            if (pass[i] && khi > klo) pass[i] = !is_known(A.known, klo, khi, key[i]);
            mk[i] = __ballot(pass[i]);
            n += __popcll(mk[i]);
          }
          if (!n) continue;
          int pos = wave_reserve(st, n, A.cap);
          if (pos < 0) break;  // the tile is redone after the workgroup made room
          const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (pass[i]) {
              const int at = pos + __popcll(mk[i] & below);
              cs[at] = tot[i];
              ck[at] = key[i];
            }
            pos += __popcll(mk[i]);
          }
        }
      }
      __syncthreads();
      if (!st->overflow) break;
      keep_best();
    }
  }
  keep_best();
  const int cnt = st->count;
  for (int i = threadIdx.x; i < cnt; i += NT) {
    A.list_s[(size_t)blockIdx.x * A.N + i] = cs[i];
    A.list_k[(size_t)blockIdx.x * A.N + i] = ck[i];
  }
  if (threadIdx.x == 0) A.list_n[blockIdx.x] = cnt;
}

// The masked dispute scan (mmsbm_scan_spread_topn_masked): the pair mask travels in the masked
// kernels' own argument struct, so SpreadArgs and the unmasked kernels do not carry it.
struct SpreadMaskedArgs : SpreadArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

// scan_spread_kernel's masked twin, restated and not a shared body, as scan_quorum_masked_kernel is.
//
// A triple is eligible only if none of its three pairs is set in the pair mask, as in scan_sweep.h
// (whose tests are restated here: this kernel does not sweep through it).  Per item the workgroup
// reads the bits (a, the item's rows) and skips the item when every row b with a < b < P is
// blocked, before the barrier, the known-key search and fill_w; otherwise row a goes to LDS behind W
// (MW words, rounded up to 2 so that the candidate buffer stays 8-byte aligned).  Per tile the
// (a, c) bits are halfword ct of that row: at 0xFFFF neither the slot loop nor the selection runs.
// The (b, c) halfwords of the lane's four rows are loaded one tile ahead (and again for a tile that
// is redone) and the blocked bits are folded into pass[i], so no blocked triple ever enters a
// candidate buffer: the workgroup's N-th best and the published bound, the seeding pass's included,
// are formed from masked-eligible candidates only and stay lower bounds of the masked N-th best.
// The cut ballot looks at scores alone: pure pruning, as without a mask.
template <int KS, int D>
__global__ __launch_bounds__(NT) void scan_spread_masked_kernel(SpreadMaskedArgs A) {
  using Sc = Score<KS>;
  constexpr int WS = Sc::WS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));
  const int RB = 16 * A.WB;
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns;
  double* lcs = W + (size_t)ns * RB * WS;  // the candidate buffer when it is in LDS
  unsigned* mrow = reinterpret_cast<unsigned*>(lcs);  // row a of the mask, before the candidate buffer
  lcs += (A.MW + 1) >> 1;
  long long* lck = reinterpret_cast<long long*>(lcs + A.cap);
  double* cs = lcs;
  long long* ck = lck;
  if (A.cand_s) {
    cs = A.cand_s + (size_t)blockIdx.x * A.cap;
    ck = A.cand_k + (size_t)blockIdx.x * A.cap;
  }
  auto keep_best = [&]() {
    if (A.cand_s) wg_keep_best(st, cs, ck, A.N, A.shared);
    else wg_keep_best(st, lcs, lck, A.N, A.shared);
  };
  if (threadIdx.x == 0) sel_init(st);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const long long PP = (long long)P;

  for (long long q = (long long)blockIdx.x * A.stride; q < PP * nbq; q += (long long)gridDim.x * A.stride) {
    const int a = (int)(q / nbq), bq = (int)(q % nbq);
    if (a >= P - 2 || bq * RB + RB - 1 <= a || bq * RB >= P - 1) continue;  // no a < b < c here
    {
      // the (a, b) bits of the item's rows: RB = 16, 32 or 64 bits from bit bq RB of row a on
      const int MW = A.MW, r0 = bq * RB, w0 = r0 >> 5;
      const unsigned* __restrict__ ra = A.mask + (size_t)a * MW;
      unsigned long long bits = (unsigned long long)ra[w0] >> (r0 & 31);  // w0 < MW: r0 < P - 1
      if (RB == 64 && w0 + 1 < MW) bits |= (unsigned long long)ra[w0 + 1] << 32;
      const int lo = max(a + 1, r0) - r0, hi = min(P, r0 + RB) - r0;  // 0 <= lo < hi <= RB, bits inside row a
      const unsigned long long need = (hi >= 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1);
      if ((bits & need) == need) continue;  // workgroup-uniform: every pair (a, b) of the item is blocked
    }
    __syncthreads();  // the previous item's W (and mask row) is read
    for (int i = threadIdx.x; i < A.MW; i += NT) mrow[i] = A.mask[(size_t)a * A.MW + i];
    if (threadIdx.x == 0) {
      const unsigned long long g = __hip_atomic_load(A.shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st->gthr = g ? __longlong_as_double((long long)g) : neg_inf();
    }
    if (threadIdx.x == 64 && A.n_known > 0) {  // the known keys whose first gene is a
      st->klo = lower_bound(A.known, 0, A.n_known, (long long)a * PP * PP);
      st->khi = lower_bound(A.known, st->klo, A.n_known, (long long)(a + 1) * PP * PP);
    }
    Sc::fill_w(W, A.T, A.thT, a, bq, RB, ns, K, P, P16);
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1 && b0 + 15 > a;
    int ct = bq * A.WB + wc;
    while (ct < btile) ct += CW;  // every c of those tiles is below every b
    const long long klo = st->klo, khi = st->khi;
    unsigned abm = 0;                // bit i: the pair (a, b0 + kk + 4 i) is blocked
    unsigned bcn[4] = {0, 0, 0, 0};  // the next tile's (b, c) halfwords, in flight
    const unsigned short* mrow16 = reinterpret_cast<const unsigned short*>(mrow);
    // halfword ct of mask rows b0 + kk + 4 i: inside the mask for a wave that is on (rows <= b0 + 15 <
    // P16, halfwords ct < P16 / 16 <= 2 MW)
    const unsigned bc_off = (unsigned)(b0 + kk) * (unsigned)A.MW * 4u;
    auto load_bc = [&](unsigned (&h)[4], int ct) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        h[i] = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(A.mask) +
                                                        (size_t)(16 * i) * A.MW + (bc_off + 2u * (unsigned)ct));
    };
    if (wave_on) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = b0 + kk + 4 * i;
        abm |= ((mrow[b >> 5] >> (b & 31)) & 1u) << i;
      }
    }
    for (;;) {
      // the thresholds change only when the workgroup sorts its buffer (behind a barrier)
      const double thr_s = st->thr_s, gthr = st->gthr;
      const long long thr_k = st->thr_k;
      const double cut = fmax(thr_s, gthr);
      if (wave_on) {
        if (ct < nct) load_bc(bcn, ct);  // also for a tile that is redone
        for (; ct < nct; ct += CW) {
          const int c0 = ct * 16;
          const unsigned ac = mrow16[ct];
          const bool dead = ac == 0xFFFFu;  // every pair (a, c) of the tile is blocked (wave-uniform)
          unsigned blk = abm | (((ac >> m) & 1u) ? 0xFu : 0u);  // bit i: element i of the tile is blocked
#pragma unroll
          for (int i = 0; i < 4; ++i) blk |= ((bcn[i] >> m) & 1u) << i;
          if (ct + CW < nct) load_bc(bcn, ct + CW);
          if (dead) continue;  // no slot loop, no selection
          const d4v tot = Sc::template tile_spread<D>(W, A.thT, ns, RB, P16, wb, c0, m, kk);
          // lane holds d[b0 + kk + 4 i][c0 + m]; from here on scan_kernel's selection
          if (!__ballot(tot[0] >= cut || tot[1] >= cut || tot[2] >= cut || tot[3] >= cut)) continue;
          const int c = c0 + m;
          bool pass[4];
          long long key[4];
          unsigned long long mk[4];
          int n = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + kk + 4 * i;
            key[i] = ((long long)a * PP + b) * PP + c;
            pass[i] = a < b && b < c && c < P && !(tot[i] < gthr) && before(tot[i], key[i], thr_s, thr_k);
            pass[i] = pass[i] && !((blk >> i) & 1u);
            if (pass[i] && khi > klo) pass[i] = !is_known(A.known, klo, khi, key[i]);
            mk[i] = __ballot(pass[i]);
            n += __popcll(mk[i]);
          }
          if (!n) continue;
          int pos = wave_reserve(st, n, A.cap);
          if (pos < 0) break;  // the tile is redone after the workgroup made room
          const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            if (pass[i]) {
              const int at = pos + __popcll(mk[i] & below);
              cs[at] = tot[i];
              ck[at] = key[i];
            }
            pos += __popcll(mk[i]);
          }
        }
      }
      __syncthreads();
      if (!st->overflow) break;
      keep_best();
    }
  }
  keep_best();
  const int cnt = st->count;
  for (int i = threadIdx.x; i < cnt; i += NT) {
    A.list_s[(size_t)blockIdx.x * A.N + i] = cs[i];
    A.list_k[(size_t)blockIdx.x * A.N + i] = ck[i];
  }
  if (threadIdx.x == 0) A.list_n[blockIdx.x] = cnt;
}

// ------------------------------------------------------------------------------------------
// Host side: the plan, the merge and the pass loop are scan_topn.h
// ------------------------------------------------------------------------------------------

// f(std::integral_constant<int, D>{}) for D = trim + 1 in [1, SPREAD_MAX_TRIM + 1]
template <class F>
int dispatch_depth(int d, F&& f) {
  switch (d) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// Both entry points; `masked`: mmsbm_scan_spread_topn_masked, whose mask must not be null.
int spread_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
                bool masked, const double* theta, const double* pr, int32_t sample, int32_t trim, int32_t N,
                void* ws, int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count,
                void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  TopNPlan p;
  int rc = make_plan(c, "the dispute scan", N, &p);
  if (rc) return rc;
  if (!order || !theta || !pr || !out_scores || !out_ids || !out_count)
    return fail(MMSBM_ERR_INVALID, "null pointer");
  const ScanShape& sh = p.sh;
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "the dispute scan", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "the dispute scan", "mmsbm_scan_spread_workspace_bytes", known, n_known, sample, ws,
                       ws_bytes, p.total, &ns, &s0)))
    return rc;
  if (sample >= 0)
    return fail(MMSBM_ERR_INVALID, "sample=%d: one restart has no spread, the dispute scan takes sample = -1",
                sample);
  if (ns < 2)
    return fail(MMSBM_ERR_INVALID, "%d active slot: one restart has no spread, the dispute scan needs two", ns);
  if (trim < 0 || ns - 2 * (long long)trim < 2)
    return fail(MMSBM_ERR_INVALID, "trim=%d outside [0, %d]: %d scored slots must keep two scores", trim,
                (ns - 2) / 2, ns);
  if (trim > SPREAD_MAX_TRIM)
    return fail(MMSBM_ERR_UNSUPPORTED,
                "trim=%d of %d slots needs two sorted lists of depth %d, above the cap of trim %d "
                "(mmsbm_scan_spread_max_trim)",
                trim, ns, trim + 1, SPREAD_MAX_TRIM);
  if ((rc = pick_wb(sh, "the dispute scan", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  // the masked kernel's mask row lies in front of the candidate buffer
  const TopNLds l = lds_sizes(p, w_bytes, sizeof(unsigned) * (size_t)((MW + 1) & ~1));
  // measurement: fewer workgroups than planned (the lists and buffers are sized for p.G)
  const long long g_env = env_override("MMSBM_SCAN_SPREAD_GRID", 0);
  const int G = g_env >= 1 ? (int)std::min<long long>(g_env, p.G) : p.G;
  hipStream_t s = (hipStream_t)stream;
  // the N-th best d_t of a subset is a lower bound of the whole's: the seeding pass as in mmsbm_scan_topn
  return run_passes(p, l.merge_lds, true, G, order, theta, pr, ns, s0, ws, out_scores, out_ids, out_count, s,
                    [&](int n_lists, int stride) {
    SpreadMaskedArgs am{};
    SpreadArgs& a = am;
    fill_common(a, p, l, ws, known, n_known, ns, WB, stride);
    am.mask = mask, am.MW = MW;
    return dispatch_ks(sh.KP / 4, [&](auto ks) {
      return dispatch_depth(trim + 1, [&](auto d) {
        constexpr int KS = decltype(ks)::value, D = decltype(d)::value;
        if (masked) return launch_lds(scan_spread_masked_kernel<KS, D>, n_lists, l.lds, s, am);
        return launch_lds(scan_spread_kernel<KS, D>, n_lists, l.lds, s, a);
      });
    });
  });
}
}  // namespace

extern "C" {

int mmsbm_scan_spread_max_trim(void) { return SPREAD_MAX_TRIM; }

int mmsbm_scan_spread_workspace_bytes(const mmsbm_ctx* c, int32_t N, int64_t* bytes) {
  return workspace_bytes(c, "the dispute scan", N, bytes);
}

int mmsbm_scan_spread_topn(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                           const double* theta, const double* pr, int32_t sample, int32_t trim, int32_t N,
                           void* ws, int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count,
                           void* stream) {
  return spread_call(c, order, known, n_known, nullptr, false, theta, pr, sample, trim, N, ws, ws_bytes,
                     out_scores, out_ids, out_count, stream);
}

int mmsbm_scan_spread_topn_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                                  const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                                  int32_t trim, int32_t N, void* ws, int64_t ws_bytes, double* out_scores,
                                  int32_t* out_ids, int64_t* out_count, void* stream) {
  return spread_call(c, order, known, n_known, mask, true, theta, pr, sample, trim, N, ws, ws_bytes,
                     out_scores, out_ids, out_count, stream);
}

}  // extern "C"
