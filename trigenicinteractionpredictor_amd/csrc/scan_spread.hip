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
// (scan_select.h, used as it is; the kernel, the merge kernel and the host loop are restated here,
// so that scan.hip's and scan_quorum.hip's instantiations stay the objects they were).  Only the tile
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

namespace {

using namespace scan_host;
using namespace scan_select;
using scan_score::scan_prep_kernel;
using scan_score::Score;
using scan_score::W_LDS_MAX;

constexpr int SPREAD_MAX_N = 4096;   // mmsbm_scan_max_n(): the scan's cap
constexpr int SPREAD_MAX_TRIM = 3;   // two sorted lists of depth 4, the quorum scan's depth
constexpr int SEED_STRIDE = 61;      // as scan.hip
constexpr int SEED_MIN_P = 200;

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
// Merge, as scan.hip's scan_merge_kernel: workgroup w keeps the best N of lists [FAN w, FAN (w + 1));
// the last level (one workgroup) writes the result: scores, gene ids in key order, count, NaN / -1
// tail.
// ------------------------------------------------------------------------------------------
struct MergeArgs {
  const double* in_s;
  const long long* in_k;
  const int* in_n;
  int n_in;
  double* out_s;      // next level's lists (null on the last level)
  long long* out_k;
  int* out_n;
  const int* order;   // last level
  double* scores;
  int* ids;
  long long* count;
  unsigned long long* shared;  // last level of the seeding pass: publish the N-th score, no output
  int N, cap, P;
};

__global__ __launch_bounds__(NT) void scan_spread_merge_kernel(MergeArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* cs = reinterpret_cast<double*>(smem + sizeof(Sel));
  long long* ck = reinterpret_cast<long long*>(cs + A.cap);
  if (threadIdx.x == 0) sel_init(st);
  __syncthreads();
  const int l0 = blockIdx.x * FAN, l1 = min(l0 + FAN, A.n_in);
  wg_merge_lists(st, cs, ck, A.in_s, A.in_k, A.in_n, l0, l1, A.N, A.cap);
  wg_keep_best(st, cs, ck, A.N, A.shared);  // seeding pass: publishes the subset's N-th score
  if (A.shared) return;
  const int cnt = st->count;
  if (A.out_s) {
    for (int i = threadIdx.x; i < cnt; i += NT) {
      A.out_s[(size_t)blockIdx.x * A.N + i] = cs[i];
      A.out_k[(size_t)blockIdx.x * A.N + i] = ck[i];
    }
    if (threadIdx.x == 0) A.out_n[blockIdx.x] = cnt;
    return;
  }
  const long long PP = A.P;
  for (int i = threadIdx.x; i < A.N; i += NT) {
    if (i < cnt) {
      const long long k = ck[i];
      A.scores[i] = cs[i];
      A.ids[3 * i] = A.order[k / (PP * PP)];
      A.ids[3 * i + 1] = A.order[(k / PP) % PP];
      A.ids[3 * i + 2] = A.order[k % PP];
    } else {
      A.scores[i] = __builtin_nan("");
      A.ids[3 * i] = A.ids[3 * i + 1] = A.ids[3 * i + 2] = -1;
    }
  }
  if (threadIdx.x == 0) *A.count = cnt;
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
struct SpreadPlan {
  ScanShape sh;
  int N, cap, G, G2;
  size_t off_thT, off_T, off_cs, off_ck, off_ls[2], off_lk[2], off_ln[2], total;
};

// As scan.hip's plan: everything that sizes the workspace follows the context's shape and N only.
int make_plan(const mmsbm_ctx* c, int N, SpreadPlan* p) {
  ScanShape& sh = p->sh;
  if (int rc = scan_shape(c, "the dispute scan", &sh)) return rc;
  if (N < 1) return fail(MMSBM_ERR_INVALID, "N=%d < 1", N);
  if (N > SPREAD_MAX_N)
    return fail(MMSBM_ERR_UNSUPPORTED, "N=%d above the scan's cap of %d", N, SPREAD_MAX_N);
  if (int rc = packed_keys_fit(sh)) return rc;
  p->N = N;
  p->cap = 512;
  while (p->cap < 2 * N) p->cap <<= 1;
  const long long per_cu = N <= 1024 ? 4 : N <= 2048 ? 2 : 1;
  const long long items = std::max<long long>(1, (long long)sh.P * (sh.P16 / 16));
  p->G = (int)std::min<long long>(per_cu * sh.ncu, items);
  p->G2 = (p->G + FAN - 1) / FAN;
  const size_t G = p->G, cap = p->cap;
  size_t off = 256;  // [0, 256): the published threshold
  score_workspace(sh, off, &p->off_thT, &p->off_T);
  p->off_cs = off, off = align256(off + sizeof(double) * G * cap);
  p->off_ck = off, off = align256(off + sizeof(long long) * G * cap);
  const size_t nl[2] = {G, (size_t)p->G2};
  for (int i = 0; i < 2; ++i) {
    p->off_ls[i] = off, off = align256(off + sizeof(double) * nl[i] * N);
    p->off_lk[i] = off, off = align256(off + sizeof(long long) * nl[i] * N);
    p->off_ln[i] = off, off = align256(off + sizeof(int) * nl[i]);
  }
  p->total = off;
  return MMSBM_OK;
}

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
  SpreadPlan p;
  int rc = make_plan(c, N, &p);
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
  const size_t cand_bytes = (size_t)p.cap * 16;
  // the masked kernel's mask row may move the candidate buffer to the workspace, which holds it anyway
  const size_t mrow_bytes = sizeof(unsigned) * (size_t)((MW + 1) & ~1);
  const bool cand_lds = sizeof(Sel) + w_bytes + mrow_bytes + cand_bytes <= (size_t)LDS_MAX;
  const int lds = (int)(sizeof(Sel) + w_bytes + mrow_bytes + (cand_lds ? cand_bytes : 0));
  const int merge_lds = (int)(sizeof(Sel) + cand_bytes);
  // measurement: fewer workgroups than planned (the lists and buffers are sized for p.G)
  const long long g_env = env_override("MMSBM_SCAN_SPREAD_GRID", 0);
  const int G = g_env >= 1 ? (int)std::min<long long>(g_env, p.G) : p.G;

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  HIP_TRY(hipMemsetAsync(w, 0, 256, s));
  int* ln[2] = {(int*)(w + p.off_ln[0]), (int*)(w + p.off_ln[1])};
  double* ls[2] = {(double*)(w + p.off_ls[0]), (double*)(w + p.off_ls[1])};
  long long* lk[2] = {(long long*)(w + p.off_lk[0]), (long long*)(w + p.off_lk[1])};
  if (sh.P >= 3) {
    scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                     (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P, sh.P16, s0);
    HIP_TRY(hipGetLastError());
  }
  // Pass 0 (large P only) seeds the bound and pass 1 scans every item, as in mmsbm_scan_topn: the
  // N-th best d_t of a subset is a lower bound of the whole's.  The bound only prunes.
  for (int pass = sh.P >= SEED_MIN_P ? 0 : 1; pass < 2; ++pass) {
    const bool seeding = pass == 0;
    int n_lists = 0;
    if (sh.P >= 3) {
      SpreadArgs a{};
      a.thT = (const double*)(w + p.off_thT);
      a.T = (const double*)(w + p.off_T);
      a.known = (const long long*)known;
      a.n_known = n_known;
      a.cand_s = cand_lds ? nullptr : (double*)(w + p.off_cs);
      a.cand_k = cand_lds ? nullptr : (long long*)(w + p.off_ck);
      a.list_s = ls[0];
      a.list_k = lk[0];
      a.list_n = ln[0];
      a.shared = (unsigned long long*)w;
      a.K = sh.K, a.P = sh.P, a.P16 = sh.P16, a.ns = ns, a.N = N, a.cap = p.cap, a.WB = WB;
      a.stride = seeding ? SEED_STRIDE : 1;
      n_lists = seeding ? std::min(G, sh.ncu) : G;
      SpreadMaskedArgs am{};
      static_cast<SpreadArgs&>(am) = a;
      am.mask = mask, am.MW = MW;
      rc = dispatch_ks(sh.KP / 4, [&](auto ks) {
        return dispatch_depth(trim + 1, [&](auto d) {
          constexpr int KS = decltype(ks)::value, D = decltype(d)::value;
          if (masked) return launch_lds(scan_spread_masked_kernel<KS, D>, n_lists, lds, s, am);
          return launch_lds(scan_spread_kernel<KS, D>, n_lists, lds, s, a);
        });
      });
      if (rc) return rc;
    }
    int cur = 0;
    for (;;) {
      const bool last = n_lists <= FAN;
      MergeArgs ma{};
      ma.in_s = ls[cur], ma.in_k = lk[cur], ma.in_n = ln[cur], ma.n_in = n_lists;
      if (!last) ma.out_s = ls[cur ^ 1], ma.out_k = lk[cur ^ 1], ma.out_n = ln[cur ^ 1];
      ma.order = order, ma.scores = out_scores, ma.ids = out_ids, ma.count = (long long*)out_count;
      ma.shared = (seeding && last) ? (unsigned long long*)w : nullptr;
      ma.N = N, ma.cap = p.cap, ma.P = std::max(sh.P, 1);
      const int n_out = last ? 1 : (n_lists + FAN - 1) / FAN;
      if ((rc = launch_lds(scan_spread_merge_kernel, n_out, merge_lds, s, ma))) return rc;
      if (last) break;
      n_lists = n_out;
      cur ^= 1;
    }
  }
  return MMSBM_OK;
}
}  // namespace

extern "C" {

int mmsbm_scan_spread_max_trim(void) { return SPREAD_MAX_TRIM; }

int mmsbm_scan_spread_workspace_bytes(const mmsbm_ctx* c, int32_t N, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  SpreadPlan p;
  int rc = make_plan(c, N, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
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
