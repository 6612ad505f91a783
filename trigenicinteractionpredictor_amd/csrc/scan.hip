// scan.hip — MI355X (gfx950) kernels + C ABI (include/mmsbm.h, mmsbm_scan_*) of the genome-wide
// scan: the exact top N of do_prediction (:530-547) over every triple of distinct genes.
//
// A triple is three rank positions a < b < c of the genes sorted by str(id) (the reference's key
// order, :349-358); its score is P(r = 1) = sum th_i[x] th_j[y] th_k[z] p_1[x][y][z] with
// i, j, k = order[a], order[b], order[c].  With Th' = theta in rank order the scores factor
// through the first gene (the engine's pivot factorisation, one level up):
//   T_a[y][z] = sum_x Th'[a][x] p_1[x][y][z]            K^3 per gene         (scan_prep_kernel)
//   W_a[b][z] = sum_y Th'[b][y] T_a[y][z]               K^2 per (a, b)       (scan_kernel, LDS)
//   S_a[b][c] = sum_z W_a[b][z] Th'[c][z]               K per triple         (v_mfma_f64_16x16x4)
// so the score phase is a batched FP64 GEMM of inner size K: 2 K C(P,3) FLOP per sample.
//
// scan_kernel: a work item is (a, a block of 16 WB rows b); the workgroup's 4 waves hold WB b-tiles
// x 4 / WB interleaved c-tiles, W_a of the item's rows in LDS (every sample of the ensemble), the
// Th' operand k-major from global (the same words for the waves that share a c-tile).  For the
// ensemble each sample's tile is accumulated from zero and the tiles are added in slot order, then
// divided by the sample count.  Items go to workgroups round-robin (no workgroup waits on another).
//
// Selection: every workgroup keeps a candidate buffer (LDS when it fits, else workspace) of a
// power-of-two capacity >= 2N.  A wave appends, by ballot compaction and one LDS compare-exchange
// that reserves the whole tile's entries, every eligible score not behind the workgroup's
// threshold; the exclusion test (binary search in the sorted known keys) runs only for those.
// When a reservation does not fit the workgroup sorts the buffer (bitonic, total order: score
// descending, packed key ascending), keeps the best N, and raises its threshold to the N-th.  The
// N-th score is also published with an agent-scope atomic max (positive doubles order as integers)
// and read once per item: a workgroup's N-th best is a lower bound of the global N-th, so pruning
// scores strictly below it never drops a member of the result, seen or not.  For P >= 200 a seeding
// pass runs first: the same scan and merge over every 61st item, whose exact N-th score (a subset's
// N-th best is such a lower bound too) is published before the full pass starts, so the full pass
// appends about 61 N candidates in all instead of filling every buffer from nothing.  At the end each
// workgroup writes its sorted best N; scan_topn.h's merge kernel (own launches, fan-in 32) merges
// the lists with the same buffer and order.  The exact top N under a total order is unique: the
// result does not depend on the grid, the arrival order or the batch.  Scores are never combined by
// atomics and every sum has a fixed order.  The selection machinery (order, buffer, keep-best-N,
// merge) is scan_select.h, shared with the partner scan (partners.hip); the score phase (prep, W
// rows, the MFMA chain of a tile, the ensemble's sum and division) is scan_score.h, shared with the
// sweep of the score census and the pair census (scan_sweep.h), whose scores therefore carry this
// kernel's bits; the host prologue (shape, checks, launch, dispatch on K) is scan_host.h, shared by
// all four.  The plan and its workspace layout, the LDS sizing, the merge kernel and the host loop
// over the seeding pass, the full pass and the merge levels are scan_topn.h, shared with the quorum
// scan (scan_quorum.hip) and the dispute scan (scan_spread.hip): this file holds the kernel, its
// pair-masked twin (scan_masked_kernel, mmsbm_scan_topn_masked), the call's own checks and the
// kernels' launch.  MMSBM_SCAN_GRID (measurement) runs fewer workgroups than planned, as
// MMSBM_SCAN_QUORUM_GRID does for the quorum scan: the list does not depend on it.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
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

// ------------------------------------------------------------------------------------------
// Scan
// ------------------------------------------------------------------------------------------
struct ScanArgs {
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
  int K, P, P16, ns, N, cap, WB, select;
  int stride;                 // 1: every item; > 1: the seeding pass over every stride-th item
};

template <int KS>
__global__ __launch_bounds__(NT) void scan_kernel(ScanArgs A) {
  using Sc = Score<KS>;  // the score phase (scan_score.h)
  constexpr int WS = Sc::WS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));
  const int RB = 16 * A.WB;                     // rows b of one item
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns;
  double* lcs = W + (size_t)ns * RB * WS;  // the candidate buffer when it is in LDS
  long long* lck = reinterpret_cast<long long*>(lcs + A.cap);
  double* cs = lcs;
  long long* ck = lck;
  if (A.cand_s) {
    cs = A.cand_s + (size_t)blockIdx.x * A.cap;
    ck = A.cand_k + (size_t)blockIdx.x * A.cap;
  }
  // the sort, on the buffer where it is (a workgroup-uniform branch around the inlined copies)
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
  const double inv_div = (double)ns;

  // items round-robin over the workgroups; the seeding pass takes every A.stride-th item only
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
    Sc::fill_w(W, A.T, A.thT, a, bq, RB, ns, K, P, P16);  // W_a of the item's rows, every sample
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1 && b0 + 15 > a;
    double areg[KS];
    if (wave_on && ns == 1) Sc::load_a(areg, W, wb, m, kk);
    int ct = bq * A.WB + wc;
    while (ct < btile) ct += CW;  // every c of those tiles is below every b
    const long long klo = st->klo, khi = st->khi;
    for (;;) {
      // the thresholds change only when the workgroup sorts its buffer (behind a barrier)
      const double thr_s = st->thr_s, gthr = st->gthr;
      const long long thr_k = st->thr_k;
      const double cut = fmax(thr_s, gthr);
      if (wave_on) {
        double bnext[KS];  // single sample: the next tile's Th' operand is in flight
        if (ns == 1 && ct < nct) Sc::load_b(bnext, A.thT, P16, ct * 16, m, kk);
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
            tot = Sc::tile_mean(W, A.thT, ns, RB, P16, wb, c0, m, kk, inv_div);
          }
          if (!A.select) continue;
          // lane holds S[b0 + kk + 4 i][c0 + m].  First the score alone against the larger of the
          // two bounds (equal scores stay in: the key decides below); nearly every tile ends here
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

// The masked scan (mmsbm_scan_topn_masked): the pair mask travels in the masked kernel's own
// argument struct, so ScanArgs and scan_kernel are what they were.
struct ScanMaskedArgs : ScanArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

// scan_kernel's masked twin, restated and not a shared body, as scan_quorum.hip restates its own (a
// shared body moved the register allocation of the unmasked instantiations there; DESIGN.md holds
// the figures that show scan_kernel's unchanged).
//
// A triple is eligible only if none of its three pairs is set in the pair mask.  Per item the
// workgroup reads the bits (a, the item's rows) and skips the item when every row b with a < b < P is
// blocked, before the barrier, the known-key search and fill_w; otherwise row a goes to LDS behind W
// (MW words, rounded up to 2 so that the candidate buffer stays 8-byte aligned).  Per tile the (a, c)
// bits are halfword ct of that row: at 0xFFFF neither the MFMA chain nor the selection runs.  The
// (b, c) halfwords of the lane's four rows are loaded one tile ahead, with the Th' operand (and again
// for a tile that is redone), and the blocked bits are folded into pass[i], so no blocked triple ever
// enters a candidate buffer: the workgroup's N-th best and the published bound, the seeding pass's
// included, are formed from masked-eligible candidates only and stay lower bounds of the masked N-th
// best.  The cut ballot looks at scores alone: pure pruning, as without a mask.  The score phase is
// scan_kernel's, so a listed score carries the bits the unmasked scan gives that triple.
//
// ENS: the ensemble (ns > 1, tile_mean) and the single sample (tile_one on register-resident
// operands) are two instantiations, so neither carries the other's registers: every instantiation
// runs at the waves per SIMD of its unmasked twin or one more.  KS <= 3 carry a floor of 4 waves per
// SIMD, which scan_kernel<1..3> reach on their own (the grid is 4 workgroups per compute unit);
// under it they spill no VGPR and use no scratch (profiles/scan_topn_masked_resources.txt; the
// measurements with and without are in DESIGN.md).
template <int KS, bool ENS>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(KS <= 3 ? 4 : 1, 4))) void scan_masked_kernel(
    ScanMaskedArgs A) {
  using Sc = Score<KS>;  // the score phase (scan_score.h)
  constexpr int WS = Sc::WS;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));
  const int RB = 16 * A.WB;                     // rows b of one item
  const int P = A.P, P16 = A.P16, K = A.K, ns = ENS ? A.ns : 1;
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
  const double inv_div = (double)ns;

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
    Sc::fill_w(W, A.T, A.thT, a, bq, RB, ns, K, P, P16);  // W_a of the item's rows, every sample
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1 && b0 + 15 > a;
    double areg[KS];
    if (!ENS && wave_on) Sc::load_a(areg, W, wb, m, kk);
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
        double bnext[KS];  // single sample: the next tile's Th' operand is in flight
        if (!ENS && ct < nct) Sc::load_b(bnext, A.thT, P16, ct * 16, m, kk);
        if (ct < nct) load_bc(bcn, ct);  // also for a tile that is redone
        for (; ct < nct; ct += CW) {
          const int c0 = ct * 16;
          d4v tot;
          const unsigned ac = mrow16[ct];
          const bool dead = ac == 0xFFFFu;  // every pair (a, c) of the tile is blocked (wave-uniform)
          unsigned blk = abm | (((ac >> m) & 1u) ? 0xFu : 0u);  // bit i: element i of the tile is blocked
#pragma unroll
          for (int i = 0; i < 4; ++i) blk |= ((bcn[i] >> m) & 1u) << i;
          if (ct + CW < nct) load_bc(bcn, ct + CW);
          if constexpr (!ENS) {
            double bcur[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
            if (ct + CW < nct) Sc::load_b(bnext, A.thT, P16, c0 + 16 * CW, m, kk);
            if (dead) continue;
            tot = Sc::tile_one(areg, bcur);
          } else {
            if (dead) continue;  // no MFMA chain, no selection
            tot = Sc::tile_mean(W, A.thT, ns, RB, P16, wb, c0, m, kk, inv_div);
          }
          if (!A.select) continue;
          // lane holds S[b0 + kk + 4 i][c0 + m]; from here on scan_kernel's selection
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

// Both entry points; `masked`: mmsbm_scan_topn_masked, whose mask must not be null.
int scan_call(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known, const uint32_t* mask,
              bool masked, const double* theta, const double* pr, int32_t sample, int32_t N, void* ws,
              int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  TopNPlan p;
  int rc = make_plan(c, "scan", N, &p);
  if (rc) return rc;
  if (!order || !theta || !pr || !out_scores || !out_ids || !out_count)
    return fail(MMSBM_ERR_INVALID, "null pointer");
  const ScanShape& sh = p.sh;
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "scan", mask, &MW))) return rc;
  int ns, s0, WB;
  size_t w_bytes;
  if ((rc = check_call(sh, "scan", "mmsbm_scan_workspace_bytes", known, n_known, sample, ws, ws_bytes, p.total, &ns,
                       &s0)))
    return rc;
  if ((rc = pick_wb(sh, "scan", 1, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  // the masked kernel's mask row lies in front of the candidate buffer
  const TopNLds l = lds_sizes(p, w_bytes, sizeof(unsigned) * (size_t)((MW + 1) & ~1));
  const bool select = env_override("MMSBM_SCAN_SELECT", 1) != 0;  // measurement: the bare score phase
  // measurement: fewer workgroups than planned (the lists and buffers are sized for p.G)
  const long long g_env = env_override("MMSBM_SCAN_GRID", 0);
  const int G = g_env >= 1 ? (int)std::min<long long>(g_env, p.G) : p.G;
  hipStream_t s = (hipStream_t)stream;
  // without the selection there is no bound to seed
  return run_passes(p, l.merge_lds, select, G, order, theta, pr, ns, s0, ws, out_scores, out_ids, out_count, s,
                    [&](int n_lists, int stride) {
    ScanMaskedArgs am{};
    ScanArgs& a = am;
    fill_common(a, p, l, ws, known, n_known, ns, WB, stride);
    a.select = select;
    am.mask = mask, am.MW = MW;
    return dispatch_ks(sh.KP / 4, [&](auto ks) {
      constexpr int KS = decltype(ks)::value;
      if (masked) {
        if (ns > 1) return launch_lds(scan_masked_kernel<KS, true>, n_lists, l.lds, s, am);
        return launch_lds(scan_masked_kernel<KS, false>, n_lists, l.lds, s, am);
      }
      return launch_lds(scan_kernel<KS>, n_lists, l.lds, s, a);
    });
  });
}

}  // namespace

// ------------------------------------------------------------------------------------------
// Host side: the plan, the merge and the pass loop are scan_topn.h
// ------------------------------------------------------------------------------------------

extern "C" {

int mmsbm_scan_max_n(void) { return TOPN_MAX_N; }

int mmsbm_scan_workspace_bytes(const mmsbm_ctx* c, int32_t N, int64_t* bytes) {
  return workspace_bytes(c, "scan", N, bytes);
}

int mmsbm_scan_topn(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                    const double* theta, const double* pr, int32_t sample, int32_t N, void* ws,
                    int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count,
                    void* stream) {
  return scan_call(c, order, known, n_known, nullptr, false, theta, pr, sample, N, ws, ws_bytes, out_scores,
                   out_ids, out_count, stream);
}

int mmsbm_scan_topn_masked(mmsbm_ctx* c, const int32_t* order, const int64_t* known, int64_t n_known,
                           const uint32_t* mask, const double* theta, const double* pr, int32_t sample,
                           int32_t N, void* ws, int64_t ws_bytes, double* out_scores, int32_t* out_ids,
                           int64_t* out_count, void* stream) {
  return scan_call(c, order, known, n_known, mask, true, theta, pr, sample, N, ws, ws_bytes, out_scores, out_ids,
                   out_count, stream);
}

}  // extern "C"
