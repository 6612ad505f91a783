// partners.hip — MI355X (gfx950) kernels + C ABI (include/mmsbm.h, mmsbm_partners_*) of the partner
// scan: for each query gene, the exact top N of do_prediction (:530-547) over every pair of other
// genes it can form a triple with.
//
// Notation as in scan.hip: Th' = theta in rank order (ids sorted by str(id)), p_1 the rating-1
// lattice, a triple three rank positions sorted ascending.  For a query at position q the candidates
// are the pairs b < c with b, c != q, and the score factors through the query's slot of p_1:
//   q < b < c:  S = Th'[b] T1_q Th'[c]^T,  T1_q[y][z] = sum_x Th'[q][x] p_1[x][y][z]
//   b < q < c:  S = Th'[b] T2_q Th'[c]^T,  T2_q[x][z] = sum_y Th'[q][y] p_1[x][y][z]
//   b < c < q:  S = Th'[b] T3_q Th'[c]^T,  T3_q[x][y] = sum_z Th'[q][z] p_1[x][y][z]
// so a query is two triangles and a rectangle of one P x P matrix, each a GEMM of inner size K:
//   Tm_q               K^3 per query and matrix      (partners_prep_kernel)
//   Wm[b] = Th'[b] Tm  K^2 per (q, b, m)             (partners_kernel, LDS)
//   S[b][c] = Wm[b] . Th'[c]                         (v_mfma_f64_16x16x4)
// A row b > q needs W1 only, a row b < q W2 (for c > q) and W3 (for c < q), so two W rows per b
// cover the three regions: U[b] = W1[b] (b > q) or W2[b] (b < q) for every c > q, L[b] = W3[b] for
// every c < q.
//
// partners_kernel: a work item is (query, a block of 16 WB rows b, a chunk of c-tiles); the row
// block holds U and L of its rows in LDS (every sample of the ensemble).  A 16 x 16 tile runs the
// U chain, the L chain, or both on the tiles the query's column crosses, and each lane keeps the
// chain of its own column (c > q: U, c < q: L), so a score's bits follow from (q, b, c) alone.  Query i owns workgroups [i gpq, (i + 1) gpq): gpq follows the device size over
// Q, so one query spreads over the device and P queries get a workgroup or two each; the c chunks
// exist only to cut one query into enough items.  Selection is the scan's (scan_select.h), per
// query: every workgroup keeps its best N in LDS and publishes its N-th score to the query's word
// (a subset's N-th best is a lower bound of the query's N-th), partners_merge_kernel merges a
// query's lists (fan-in 32, at most two levels) and writes its row.  The exact top N under a total
// order is unique, no score is formed by an atomic and every sum has a fixed order: a query's row
// does not depend on Q, the other queries, the grid or the batch.
//
// partners_masked_kernel (mmsbm_partners_topn_masked) is partners_kernel's pair-masked twin: the
// query's own bit row in LDS, row blocks and tiles dropped by it, the (b, c) bits per element.
// partners_stat_kernel (mmsbm_partners_stat_topn): the ensemble path's tile with an order statistic
// of the slots' own scores in the mean's place, the quorum score q_m or the spread q_{1+t} - q_{ns-t},
// from per-element sorted lists in registers; the mask is a nullable pointer.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "mmsbm.h"
#include "scan_host.h"
#include "scan_select.h"

namespace {

using namespace scan_host;
using namespace scan_select;

constexpr int PARTNERS_MAX_N = 1024;   // documented cap of N (include/mmsbm.h): the buffer stays in LDS
constexpr int MAX_GPQ = FAN * FAN;     // workgroups per query: two merge levels at most
constexpr int W_LDS_MAX = 96 * 1024;   // U and L of one row block, every sample

// ------------------------------------------------------------------------------------------
// Prep
// ------------------------------------------------------------------------------------------
// Th' k-major and zero-padded: thT[s][KP][P16].  grid (ceil(KP P16 / NT), samples).
__global__ __launch_bounds__(NT) void partners_theta_kernel(const int* __restrict__ order,
                                                            const double* __restrict__ theta,
                                                            double* __restrict__ thT, int K, int KP, int P,
                                                            int P16, int s0) {
  const int idx = blockIdx.x * NT + threadIdx.x, s = blockIdx.y;
  if (idx >= KP * P16) return;
  const int k = idx / P16, a = idx % P16;
  int g = a < P ? order[a] : -1;
  if (g < 0 || g >= P) g = -1;  // outside the table: a zero row
  thT[(size_t)s * KP * P16 + idx] = (g >= 0 && k < K) ? theta[((size_t)(s0 + s) * P + g) * K + k] : 0.0;
}

// T[s][Q][3][K][KP] of every query (zero-padded like the scan's T_a) and its rank position.
// grid (Q, samples).
__global__ __launch_bounds__(NT) void partners_prep_kernel(const int* __restrict__ order,
                                                           const int* __restrict__ queries,
                                                           const double* __restrict__ theta,
                                                           const double* __restrict__ pr,
                                                           double* __restrict__ T, int* __restrict__ qpos,
                                                           int K, int KP, int R, int P, int Q, int s0) {
  __shared__ double th[MMSBM_MAX_K];
  __shared__ int pos;
  const int qi = blockIdx.x, s = blockIdx.y;
  const int g = queries[qi];  // in [0, P): checked on the host
  const size_t K2 = (size_t)K * K, K3 = K2 * K;
  if (threadIdx.x == 0) pos = -1;
  if ((int)threadIdx.x < K) th[threadIdx.x] = theta[((size_t)(s0 + s) * P + g) * K + threadIdx.x];
  __syncthreads();
  if (s == 0) {
    for (int a = threadIdx.x; a < P; a += NT)
      if (order[a] == g) pos = a;
    __syncthreads();
    if (threadIdx.x == 0) qpos[qi] = pos;  // -1 (order is no permutation): the query has no candidate
  }
  const double* __restrict__ p1 = pr + ((size_t)(s0 + s) * R + 1) * K3;
  double* __restrict__ Tq = T + ((size_t)s * Q + qi) * 3 * K * KP;
  for (int idx = threadIdx.x; idx < 3 * K * KP; idx += NT) {
    const int mm = idx / (K * KP), i = (idx / KP) % K, j = idx % KP;
    double v = 0.0;
    if (j < K) {
      // the query's slot is contracted: slot 1 (T1[y][z]), slot 2 (T2[x][z]) or slot 3 (T3[x][y])
      const double* __restrict__ p = mm == 0 ? p1 + i * K + j : mm == 1 ? p1 + i * K2 + j : p1 + i * K2 + j * K;
      const size_t step = mm == 0 ? K2 : mm == 1 ? (size_t)K : (size_t)1;
      for (int t = 0; t < K; ++t) v = fma(th[t], p[t * step], v);
    }
    Tq[idx] = v;
  }
}

// ------------------------------------------------------------------------------------------
// Scan
// ------------------------------------------------------------------------------------------
struct PartArgs {
  const double* thT;           // [ns][KP][P16]
  const double* T;             // [ns][Q][3][K][KP]
  const int* qpos;             // [Q] rank position of each query
  const long long* known_off;  // [Q + 1] (null: no exclusion)
  const long long* known;      // each query's sorted pair keys b P + c
  double* list_s;              // per-workgroup results [Q gpq][N]
  long long* list_k;
  int* list_n;                 // [Q gpq]
  unsigned long long* shared;  // [Q] published threshold bits
  int K, P, P16, Q, ns, N, cap, WB, select;
  int gpq;                     // workgroups per query
  int ncc;                     // c chunks per row block
};

template <int KS>
__global__ __launch_bounds__(NT) void partners_kernel(PartArgs A) {
  constexpr int KP = 4 * KS, WS = KP + 2;  // W row stride: conflict-free A-operand reads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));  // [2][ns][RB][WS]: U, L
  const int RB = 16 * A.WB;
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns;
  double* cs = W + (size_t)2 * ns * RB * WS;  // the candidate buffer
  long long* ck = reinterpret_cast<long long*>(cs + A.cap);
  const int qi = blockIdx.x / A.gpq, j = blockIdx.x % A.gpq;
  const int q = A.qpos[qi];
  unsigned long long* shared = A.shared + qi;
  if (threadIdx.x == 0) {
    sel_init(st);
    if (A.known_off) {
      st->klo = A.known_off[qi];
      st->khi = A.known_off[qi + 1];
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const int CT = (nct + A.ncc - 1) / A.ncc;  // c-tiles per chunk
  const long long PP = (long long)P;
  const double inv_div = (double)ns;
  const size_t Tq = (size_t)qi * 3 * K * KP, Ts = (size_t)A.Q * 3 * K * KP;

  // the query's items round-robin over its workgroups
  for (int it = (q >= 0 && q < P) ? j : INT_MAX; it < nbq * A.ncc; it += A.gpq) {
    const int bq = it / A.ncc, cc = it % A.ncc;
    const int ct_lo = cc * CT, ct_hi = min(nct, ct_lo + CT);
    const int r0 = bq * RB;
    if (ct_lo >= ct_hi || r0 >= P - 1 || ct_hi * 16 - 1 <= r0) continue;  // no b < c here
    __syncthreads();  // the previous item's W is read
    if (threadIdx.x == 0) {
      const unsigned long long g = __hip_atomic_load(shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st->gthr = g ? __longlong_as_double((long long)g) : neg_inf();
    }
    // U = W1 of the rows above q and W2 of the rows below it, L = W3 of the rows below it (zero
    // elsewhere), every sample
    for (int idx = threadIdx.x; idx < 2 * ns * RB * KP; idx += NT) {
      const int z = idx % KP, r = (idx / KP) % RB, s = (idx / (KP * RB)) % ns, ul = idx / (KP * RB * ns);
      const int rowb = r0 + r;
      const int mm = ul ? 2 : rowb > q ? 0 : 1;
      double v = 0.0;
      if (rowb < P && rowb != q && (ul == 0 || rowb < q)) {
        const double* __restrict__ Tm = A.T + (size_t)s * Ts + Tq + (size_t)mm * K * KP + z;
        const double* __restrict__ tb = A.thT + (size_t)s * KP * P16 + rowb;
        for (int i = 0; i < K; ++i) v = fma(tb[(size_t)i * P16], Tm[i * KP], v);
      }
      W[((size_t)(ul * ns + s) * RB + r) * WS + z] = v;
    }
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1;
    const bool rows_hi = b0 + 15 > q, rows_lo = b0 < q;  // the tile has rows above / below q
    int ct = ct_lo + wc;
    if (ct < btile) ct += (btile - ct + CW - 1) / CW * CW;  // every c of those tiles is below every b
    const long long klo = st->klo, khi = st->khi;
    double areg[2][KS];  // single sample: the A operands live in registers for the whole item
    if (wave_on && ns == 1) {
#pragma unroll
      for (int ul = 0; ul < 2; ++ul)
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) areg[ul][ks] = W[((size_t)ul * RB + wb * 16 + m) * WS + 4 * ks + kk];
    }
    for (;;) {
      // the thresholds change only when the workgroup sorts its buffer (behind a barrier)
      const double thr_s = st->thr_s, gthr = st->gthr;
      const long long thr_k = st->thr_k;
      const double cut = fmax(thr_s, gthr);
      if (wave_on) {
        double bnext[KS];  // single sample: the next tile's Th' operand is in flight
        if (ns == 1 && ct < ct_hi) {
          const double* __restrict__ tc = A.thT + (size_t)kk * P16 + ct * 16 + m;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) bnext[ks] = tc[(size_t)(4 * ks) * P16];
        }
        for (; ct < ct_hi; ct += CW) {
          const int c0 = ct * 16, c = c0 + m;
          // U: some c > q (rows below q) or rows above q (all their c are); L: rows and c below q
          const bool need[2] = {rows_hi || c0 + 15 > q, rows_lo && c0 < q};
          double bcur[KS];
          if (ns == 1) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
            if (ct + CW < ct_hi) {
              const double* __restrict__ tc = A.thT + (size_t)kk * P16 + c + 16 * CW;
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) bnext[ks] = tc[(size_t)(4 * ks) * P16];
            }
          }
          d4v res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ul = 0; ul < 2; ++ul) {
            if (!need[ul]) continue;  // wave-uniform
            d4v tot = {0.0, 0.0, 0.0, 0.0};
            if (ns == 1) {
#pragma unroll
              for (int ks = 0; ks < KS; ++ks)
                tot = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[ul][ks], bcur[ks], tot, 0, 0, 0);
            } else {
              for (int s = 0; s < ns; ++s) {
                const double* __restrict__ tc = A.thT + ((size_t)s * KP + kk) * P16 + c;
                const double* wr = W + ((size_t)(ul * ns + s) * RB + wb * 16 + m) * WS + kk;
                d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], tc[(size_t)(4 * ks) * P16], acc, 0, 0, 0);
                tot = s == 0 ? acc : tot + acc;  // samples added in slot order
              }
              tot = tot / inv_div;
            }
            // lane holds S[b0 + kk + 4 i][c0 + m]: keep the chain of its own column
            if ((c < q) == (ul == 1)) res = tot;
          }
          if (!A.select) {
            asm volatile("" ::"v"(res[0]), "v"(res[1]), "v"(res[2]), "v"(res[3]));  // keep the score phase live
            continue;
          }
          // first the score alone against the larger of the two bounds (equal scores stay in: the
          // key decides below); nearly every tile ends here once the buffer holds N
          if (!__ballot(res[0] >= cut || res[1] >= cut || res[2] >= cut || res[3] >= cut)) continue;
          bool pass[4];
          long long key[4];
          unsigned long long mk[4];
          int n = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + kk + 4 * i;
            // the triple's packed key, q in its sorted place
            key[i] = b > q ? ((long long)q * PP + b) * PP + c
                   : c > q ? ((long long)b * PP + q) * PP + c
                           : ((long long)b * PP + c) * PP + q;
            pass[i] = b < c && c < P && b != q && c != q && !(res[i] < gthr) &&
                      before(res[i], key[i], thr_s, thr_k);
            if (pass[i] && khi > klo) pass[i] = !is_known(A.known, klo, khi, (long long)b * PP + c);
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
              cs[at] = res[i];
              ck[at] = key[i];
            }
            pos += __popcll(mk[i]);
          }
        }
      }
      __syncthreads();
      if (!st->overflow) break;
      wg_keep_best(st, cs, ck, A.N, shared);
    }
  }
  wg_keep_best(st, cs, ck, A.N, shared);
  const int cnt = st->count;
  for (int i = threadIdx.x; i < cnt; i += NT) {
    A.list_s[(size_t)blockIdx.x * A.N + i] = cs[i];
    A.list_k[(size_t)blockIdx.x * A.N + i] = ck[i];
  }
  if (threadIdx.x == 0) A.list_n[blockIdx.x] = cnt;
}

// The masked partner scan (mmsbm_partners_topn_masked): the pair mask travels in the masked kernel's
// own argument struct, so PartArgs and partners_kernel are what they were.
struct PartMaskedArgs : PartArgs {
  const unsigned* mask;  // [P16][MW] (include/mmsbm.h, mmsbm_pair_mask_shape)
  int MW;
};

// partners_kernel's masked twin, restated and not a shared body (scan_quorum.hip says why; DESIGN.md
// holds the figures that show partners_kernel's instantiations unchanged).
//
// A candidate pair b < c of the query at q is eligible only if none of {q, b}, {q, c}, (b, c) is set
// in the pair mask (read at x < y only).  The query's own bit row: bit x of qrow is set when the pair
// {q, x} is blocked, i.e. bit x of mask row q for x > q and bit q of mask row x for x < q; bit q
// itself and the bits from P on are set too (no candidate there), so the skips below need no bounds
// of their own.  Each workgroup builds it once, 64 positions per wave and ballot, in LDS in front of
// the candidate buffer (MW words rounded up to 2: at most 2 KiB).  An item is skipped, before its
// U / L rows are formed, when every row of its block is blocked with q; a tile, before its chains,
// when halfword ct of qrow is 0xFFFF (its 16 columns are all blocked with q).  Per element the
// blocked bit is qrow[b] | qrow[c] | mask[b][c], the (b, c) halfwords of the lane's four rows loaded
// one tile ahead as scan.hip's twin loads them, and it is folded into pass[i]: no blocked candidate
// enters a buffer, so the workgroup's N-th best and the query's published bound are formed from
// masked-eligible candidates only and stay lower bounds of the query's masked N-th best.  The score
// phase is partners_kernel's, so a listed score carries the bits the unmasked call gives it.
template <int KS>
__global__ __launch_bounds__(NT) void partners_masked_kernel(PartMaskedArgs A) {
  constexpr int KP = 4 * KS, WS = KP + 2;  // W row stride: conflict-free A-operand reads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));  // [2][ns][RB][WS]: U, L
  const int RB = 16 * A.WB;
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns;
  double* cs = W + (size_t)2 * ns * RB * WS;
  unsigned* qrow = reinterpret_cast<unsigned*>(cs);  // the query's bit row, before the candidate buffer
  const int MW2 = (A.MW + 1) & ~1;
  cs += MW2 >> 1;                                    // the candidate buffer
  long long* ck = reinterpret_cast<long long*>(cs + A.cap);
  const int qi = blockIdx.x / A.gpq, j = blockIdx.x % A.gpq;
  const int q = A.qpos[qi];
  const bool q_ok = q >= 0 && q < P;
  unsigned long long* shared = A.shared + qi;
  if (threadIdx.x == 0) {
    sel_init(st);
    if (A.known_off) {
      st->klo = A.known_off[qi];
      st->khi = A.known_off[qi + 1];
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const int CT = (nct + A.ncc - 1) / A.ncc;  // c-tiles per chunk
  const long long PP = (long long)P;
  const double inv_div = (double)ns;
  const size_t Tq = (size_t)qi * 3 * K * KP, Ts = (size_t)A.Q * 3 * K * KP;

  // the query's bit row: position x of this wave's 64, words x / 32 and x / 32 + 1 from one ballot
  for (int x = threadIdx.x; x < 32 * MW2; x += NT) {
    bool on = true;  // q itself, positions from P on, a query without a position
    if (q_ok && x < P && x != q) {
      const unsigned w = x > q ? A.mask[(size_t)q * A.MW + (x >> 5)] : A.mask[(size_t)x * A.MW + (q >> 5)];
      on = (w >> ((x > q ? x : q) & 31)) & 1u;
    }
    const unsigned long long bal = __ballot(on);
    if (lane == 0) {
      qrow[x >> 5] = (unsigned)bal;
      qrow[(x >> 5) + 1] = (unsigned)(bal >> 32);
    }
  }
  __syncthreads();
  const unsigned short* qrow16 = reinterpret_cast<const unsigned short*>(qrow);

  // the query's items round-robin over its workgroups
  for (int it = q_ok ? j : INT_MAX; it < nbq * A.ncc; it += A.gpq) {
    const int bq = it / A.ncc, cc = it % A.ncc;
    const int ct_lo = cc * CT, ct_hi = min(nct, ct_lo + CT);
    const int r0 = bq * RB;
    if (ct_lo >= ct_hi || r0 >= P - 1 || ct_hi * 16 - 1 <= r0) continue;  // no b < c here
    {
      // the {q, b} bits of the item's rows: RB = 16, 32 or 64 bits of qrow from bit r0 on
      const int w0 = r0 >> 5;
      unsigned long long bits = (unsigned long long)qrow[w0] >> (r0 & 31);  // w0 < MW: r0 < P - 1
      if (RB == 64 && w0 + 1 < MW2) bits |= (unsigned long long)qrow[w0 + 1] << 32;
      const int hi = min(P, r0 + RB) - r0;  // 0 < hi <= RB
      const unsigned long long need = hi >= 64 ? ~0ull : (1ull << hi) - 1;
      if ((bits & need) == need) continue;  // workgroup-uniform: every row of the block is blocked with q
    }
    __syncthreads();  // the previous item's W is read
    if (threadIdx.x == 0) {
      const unsigned long long g = __hip_atomic_load(shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st->gthr = g ? __longlong_as_double((long long)g) : neg_inf();
    }
    // U = W1 of the rows above q and W2 of the rows below it, L = W3 of the rows below it (zero
    // elsewhere), every sample
    for (int idx = threadIdx.x; idx < 2 * ns * RB * KP; idx += NT) {
      const int z = idx % KP, r = (idx / KP) % RB, s = (idx / (KP * RB)) % ns, ul = idx / (KP * RB * ns);
      const int rowb = r0 + r;
      const int mm = ul ? 2 : rowb > q ? 0 : 1;
      double v = 0.0;
      if (rowb < P && rowb != q && (ul == 0 || rowb < q)) {
        const double* __restrict__ Tm = A.T + (size_t)s * Ts + Tq + (size_t)mm * K * KP + z;
        const double* __restrict__ tb = A.thT + (size_t)s * KP * P16 + rowb;
        for (int i = 0; i < K; ++i) v = fma(tb[(size_t)i * P16], Tm[i * KP], v);
      }
      W[((size_t)(ul * ns + s) * RB + r) * WS + z] = v;
    }
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1;
    const bool rows_hi = b0 + 15 > q, rows_lo = b0 < q;  // the tile has rows above / below q
    int ct = ct_lo + wc;
    if (ct < btile) ct += (btile - ct + CW - 1) / CW * CW;  // every c of those tiles is below every b
    const long long klo = st->klo, khi = st->khi;
    double areg[2][KS];  // single sample: the A operands live in registers for the whole item
    unsigned qbm = 0;                // bit i: the pair {q, b0 + kk + 4 i} is blocked
    unsigned bcn[4] = {0, 0, 0, 0};  // the next tile's (b, c) halfwords, in flight
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
        qbm |= ((qrow[b >> 5] >> (b & 31)) & 1u) << i;
      }
      if (ns == 1) {
#pragma unroll
        for (int ul = 0; ul < 2; ++ul)
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) areg[ul][ks] = W[((size_t)ul * RB + wb * 16 + m) * WS + 4 * ks + kk];
      }
    }
    for (;;) {
      // the thresholds change only when the workgroup sorts its buffer (behind a barrier)
      const double thr_s = st->thr_s, gthr = st->gthr;
      const long long thr_k = st->thr_k;
      const double cut = fmax(thr_s, gthr);
      if (wave_on) {
        double bnext[KS];  // single sample: the next tile's Th' operand is in flight
        if (ns == 1 && ct < ct_hi) {
          const double* __restrict__ tc = A.thT + (size_t)kk * P16 + ct * 16 + m;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks) bnext[ks] = tc[(size_t)(4 * ks) * P16];
        }
        if (ct < ct_hi) load_bc(bcn, ct);  // also for a tile that is redone
        for (; ct < ct_hi; ct += CW) {
          const int c0 = ct * 16, c = c0 + m;
          // U: some c > q (rows below q) or rows above q (all their c are); L: rows and c below q
          const bool need[2] = {rows_hi || c0 + 15 > q, rows_lo && c0 < q};
          const unsigned qc = qrow16[ct];
          const bool dead = qc == 0xFFFFu;  // every pair {q, c} of the tile is blocked (wave-uniform)
          unsigned blk = qbm | (((qc >> m) & 1u) ? 0xFu : 0u);  // bit i: element i of the tile is blocked
#pragma unroll
          for (int i = 0; i < 4; ++i) blk |= ((bcn[i] >> m) & 1u) << i;
          if (ct + CW < ct_hi) load_bc(bcn, ct + CW);
          double bcur[KS];
          if (ns == 1) {
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
            if (ct + CW < ct_hi) {
              const double* __restrict__ tc = A.thT + (size_t)kk * P16 + c + 16 * CW;
#pragma unroll
              for (int ks = 0; ks < KS; ++ks) bnext[ks] = tc[(size_t)(4 * ks) * P16];
            }
          }
          if (dead) continue;  // no chain, no selection
          d4v res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
          for (int ul = 0; ul < 2; ++ul) {
            if (!need[ul]) continue;  // wave-uniform
            d4v tot = {0.0, 0.0, 0.0, 0.0};
            if (ns == 1) {
#pragma unroll
              for (int ks = 0; ks < KS; ++ks)
                tot = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[ul][ks], bcur[ks], tot, 0, 0, 0);
            } else {
              for (int s = 0; s < ns; ++s) {
                const double* __restrict__ tc = A.thT + ((size_t)s * KP + kk) * P16 + c;
                const double* wr = W + ((size_t)(ul * ns + s) * RB + wb * 16 + m) * WS + kk;
                d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int ks = 0; ks < KS; ++ks)
                  acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], tc[(size_t)(4 * ks) * P16], acc, 0, 0, 0);
                tot = s == 0 ? acc : tot + acc;  // samples added in slot order
              }
              tot = tot / inv_div;
            }
            // lane holds S[b0 + kk + 4 i][c0 + m]: keep the chain of its own column
            if ((c < q) == (ul == 1)) res = tot;
          }
          if (!A.select) {
            asm volatile("" ::"v"(res[0]), "v"(res[1]), "v"(res[2]), "v"(res[3]));  // keep the score phase live
            continue;
          }
          // first the score alone against the larger of the two bounds (equal scores stay in: the
          // key decides below); nearly every tile ends here once the buffer holds N
          if (!__ballot(res[0] >= cut || res[1] >= cut || res[2] >= cut || res[3] >= cut)) continue;
          bool pass[4];
          long long key[4];
          unsigned long long mk[4];
          int n = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + kk + 4 * i;
            // the triple's packed key, q in its sorted place
            key[i] = b > q ? ((long long)q * PP + b) * PP + c
                   : c > q ? ((long long)b * PP + q) * PP + c
                           : ((long long)b * PP + c) * PP + q;
            pass[i] = b < c && c < P && b != q && c != q && !(res[i] < gthr) &&
                      before(res[i], key[i], thr_s, thr_k);
            pass[i] = pass[i] && !((blk >> i) & 1u);
            if (pass[i] && khi > klo) pass[i] = !is_known(A.known, klo, khi, (long long)b * PP + c);
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
              cs[at] = res[i];
              ck[at] = key[i];
            }
            pos += __popcll(mk[i]);
          }
        }
      }
      __syncthreads();
      if (!st->overflow) break;
      wg_keep_best(st, cs, ck, A.N, shared);
    }
  }
  wg_keep_best(st, cs, ck, A.N, shared);
  const int cnt = st->count;
  for (int i = threadIdx.x; i < cnt; i += NT) {
    A.list_s[(size_t)blockIdx.x * A.N + i] = cs[i];
    A.list_k[(size_t)blockIdx.x * A.N + i] = ck[i];
  }
  if (threadIdx.x == 0) A.list_n[blockIdx.x] = cnt;
}

// ------------------------------------------------------------------------------------------
// Stat scan (mmsbm_partners_stat_topn): the top N of a query by an order statistic of the slots' own
// scores.  Restated beside its two siblings and not a shared body, so that their instantiations stay
// what they were (DESIGN.md holds the figures).  The items, the U / L rows of every slot in LDS, the
// tile walk, the keys, the eligibility, the buffer and the two bounds are partners_kernel's; the
// query's bit row, the item and tile skips and the (b, c) halfwords are partners_masked_kernel's,
// behind a nullable mask pointer (workgroup-uniform).
// Each slot's tile is formed as the ensemble path forms it (A from the slot's U / L rows, B from the
// slot's thT, every needed chain from zero over ascending k, the lane keeping the chain of its own
// column), so it is the word mmsbm_partners_topn(sample = s) lists; instead of joining a sum it is
// inserted into per-element sorted lists of depth D held in registers, `top` (the D largest,
// descending) and `bot` (the D smallest, ascending), by the max / min chain of scan_score.h with
// compile-time indices.  The wave-uniform `mode` says which list is kept and read: STAT_TOP the D-th
// largest, STAT_BOT the D-th smallest, STAT_SPREAD both and their difference, one IEEE subtraction.
// The host guarantees D <= ns (quorum) or 2 D <= ns (spread), so no start value reaches a buffer.
// Early exit (the quorum, tile_quorum's rule): from slot `first` = ns - m on and before the last
// slot, one ballot asks whether any element of the wave's tile can still reach cut = max(thr_s,
// gthr); with STAT_BOT the list's last entry, the (ns - m + 1)-th smallest so far, is below cut
// exactly when it cannot, with STAT_TOP the entries at or above cut plus the slots still to come
// fall short of m exactly then.  If none can, the tile's remaining slots are not formed.  An element
// below cut is dropped by the selection anyway, so the list does not change.  first = ns: never (the
// spread, whose value only grows as slots arrive, and MMSBM_PARTNERS_STAT_EARLY=0).
// Only the final statistic of an eligible candidate enters the buffer, so the workgroup's N-th best
// and the query's published word are lower bounds of the query's N-th best value.
// ------------------------------------------------------------------------------------------
enum : int { STAT_TOP = 0, STAT_BOT = 1, STAT_SPREAD = 2 };

struct PartStatArgs : PartMaskedArgs {  // mask = null: none (MW = 0)
  int mode;   // STAT_*
  int first;  // the first slot after which a tile may end early (ns: never)
};

template <int KS, int D>
__global__ __launch_bounds__(NT) void partners_stat_kernel(PartStatArgs A) {
  constexpr int KP = 4 * KS, WS = KP + 2;  // W row stride: conflict-free A-operand reads
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* W = reinterpret_cast<double*>(smem + sizeof(Sel));  // [2][ns][RB][WS]: U, L
  const int RB = 16 * A.WB;
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns, mode = A.mode, first = A.first;
  const bool masked = A.mask != nullptr;  // workgroup-uniform
  double* cs = W + (size_t)2 * ns * RB * WS;
  unsigned* qrow = reinterpret_cast<unsigned*>(cs);  // the query's bit row, before the candidate buffer
  const int MW2 = (A.MW + 1) & ~1;                   // 0 without a mask
  cs += MW2 >> 1;                                    // the candidate buffer
  long long* ck = reinterpret_cast<long long*>(cs + A.cap);
  const int qi = blockIdx.x / A.gpq, j = blockIdx.x % A.gpq;
  const int q = A.qpos[qi];
  const bool q_ok = q >= 0 && q < P;
  unsigned long long* shared = A.shared + qi;
  if (threadIdx.x == 0) {
    sel_init(st);
    if (A.known_off) {
      st->klo = A.known_off[qi];
      st->khi = A.known_off[qi + 1];
    }
  }

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const int CT = (nct + A.ncc - 1) / A.ncc;  // c-tiles per chunk
  const long long PP = (long long)P;
  const double inf = __builtin_huge_val();
  const size_t Tq = (size_t)qi * 3 * K * KP, Ts = (size_t)A.Q * 3 * K * KP;

  // the query's bit row: position x of this wave's 64, words x / 32 and x / 32 + 1 from one ballot
  for (int x = threadIdx.x; x < 32 * MW2; x += NT) {
    bool on = true;  // q itself, positions from P on, a query without a position
    if (q_ok && x < P && x != q) {
      const unsigned w = x > q ? A.mask[(size_t)q * A.MW + (x >> 5)] : A.mask[(size_t)x * A.MW + (q >> 5)];
      on = (w >> ((x > q ? x : q) & 31)) & 1u;
    }
    const unsigned long long bal = __ballot(on);
    if (lane == 0) {
      qrow[x >> 5] = (unsigned)bal;
      qrow[(x >> 5) + 1] = (unsigned)(bal >> 32);
    }
  }
  __syncthreads();
  const unsigned short* qrow16 = reinterpret_cast<const unsigned short*>(qrow);

  // the query's items round-robin over its workgroups
  for (int it = q_ok ? j : INT_MAX; it < nbq * A.ncc; it += A.gpq) {
    const int bq = it / A.ncc, cc = it % A.ncc;
    const int ct_lo = cc * CT, ct_hi = min(nct, ct_lo + CT);
    const int r0 = bq * RB;
    if (ct_lo >= ct_hi || r0 >= P - 1 || ct_hi * 16 - 1 <= r0) continue;  // no b < c here
    if (masked) {
      // the {q, b} bits of the item's rows: RB = 16, 32 or 64 bits of qrow from bit r0 on
      const int w0 = r0 >> 5;
      unsigned long long bits = (unsigned long long)qrow[w0] >> (r0 & 31);  // w0 < MW: r0 < P - 1
      if (RB == 64 && w0 + 1 < MW2) bits |= (unsigned long long)qrow[w0 + 1] << 32;
      const int hi = min(P, r0 + RB) - r0;  // 0 < hi <= RB
      const unsigned long long need = hi >= 64 ? ~0ull : (1ull << hi) - 1;
      if ((bits & need) == need) continue;  // workgroup-uniform: every row of the block is blocked with q
    }
    __syncthreads();  // the previous item's W is read
    if (threadIdx.x == 0) {
      const unsigned long long g = __hip_atomic_load(shared, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      st->gthr = g ? __longlong_as_double((long long)g) : neg_inf();
    }
    // U = W1 of the rows above q and W2 of the rows below it, L = W3 of the rows below it (zero
    // elsewhere), every slot
    for (int idx = threadIdx.x; idx < 2 * ns * RB * KP; idx += NT) {
      const int z = idx % KP, r = (idx / KP) % RB, s = (idx / (KP * RB)) % ns, ul = idx / (KP * RB * ns);
      const int rowb = r0 + r;
      const int mm = ul ? 2 : rowb > q ? 0 : 1;
      double v = 0.0;
      if (rowb < P && rowb != q && (ul == 0 || rowb < q)) {
        const double* __restrict__ Tm = A.T + (size_t)s * Ts + Tq + (size_t)mm * K * KP + z;
        const double* __restrict__ tb = A.thT + (size_t)s * KP * P16 + rowb;
        for (int i = 0; i < K; ++i) v = fma(tb[(size_t)i * P16], Tm[i * KP], v);
      }
      W[((size_t)(ul * ns + s) * RB + r) * WS + z] = v;
    }
    __syncthreads();

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1;
    const bool rows_hi = b0 + 15 > q, rows_lo = b0 < q;  // the tile has rows above / below q
    int ct = ct_lo + wc;
    if (ct < btile) ct += (btile - ct + CW - 1) / CW * CW;  // every c of those tiles is below every b
    const long long klo = st->klo, khi = st->khi;
    unsigned qbm = 0;                // bit i: the pair {q, b0 + kk + 4 i} is blocked
    unsigned bcn[4] = {0, 0, 0, 0};  // the next tile's (b, c) halfwords, in flight
    // halfword ct of mask rows b0 + kk + 4 i: inside the mask for a wave that is on (rows <= b0 + 15 <
    // P16, halfwords ct < P16 / 16 <= 2 MW)
    const unsigned bc_off = (unsigned)(b0 + kk) * (unsigned)A.MW * 4u;
    auto load_bc = [&](unsigned (&h)[4], int ct) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        h[i] = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(A.mask) +
                                                        (size_t)(16 * i) * A.MW + (bc_off + 2u * (unsigned)ct));
    };
    if (wave_on && masked) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = b0 + kk + 4 * i;
        qbm |= ((qrow[b >> 5] >> (b & 31)) & 1u) << i;
      }
    }
    for (;;) {
      // the thresholds change only when the workgroup sorts its buffer (behind a barrier)
      const double thr_s = st->thr_s, gthr = st->gthr;
      const long long thr_k = st->thr_k;
      const double cut = fmax(thr_s, gthr);
      if (wave_on) {
        if (masked && ct < ct_hi) load_bc(bcn, ct);  // also for a tile that is redone
        for (; ct < ct_hi; ct += CW) {
          const int c0 = ct * 16, c = c0 + m;
          // U: some c > q (rows below q) or rows above q (all their c are); L: rows and c below q
          const bool need[2] = {rows_hi || c0 + 15 > q, rows_lo && c0 < q};
          unsigned blk = 0;  // bit i: element i of the tile is blocked
          if (masked) {
            const unsigned qc = qrow16[ct];
            blk = qbm | (((qc >> m) & 1u) ? 0xFu : 0u);
#pragma unroll
            for (int i = 0; i < 4; ++i) blk |= ((bcn[i] >> m) & 1u) << i;
            if (ct + CW < ct_hi) load_bc(bcn, ct + CW);
            if (qc == 0xFFFFu) continue;  // every pair {q, c} of the tile is blocked (wave-uniform)
          }
          d4v top[D], bot[D];
#pragma unroll
          for (int jj = 0; jj < D; ++jj) {
            top[jj] = d4v{-inf, -inf, -inf, -inf};
            bot[jj] = d4v{inf, inf, inf, inf};
          }
          bool live = true;
          for (int s = 0; s < ns; ++s) {
            const double* __restrict__ tc = A.thT + ((size_t)s * KP + kk) * P16 + c;
            double bv[KS];
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) bv[ks] = tc[(size_t)(4 * ks) * P16];
            d4v sc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int ul = 0; ul < 2; ++ul) {
              if (!need[ul]) continue;  // wave-uniform
              const double* wr = W + ((size_t)(ul * ns + s) * RB + wb * 16 + m) * WS + kk;
              d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
              for (int ks = 0; ks < KS; ++ks)
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], bv[ks], acc, 0, 0, 0);
              // lane holds S[b0 + kk + 4 i][c0 + m]: keep the chain of its own column
              if ((c < q) == (ul == 1)) sc = acc;
            }
            // each list keeps the better of the two, x carries the other on
            if (mode != STAT_BOT) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                double x = sc[i];
#pragma unroll
                for (int jj = 0; jj < D; ++jj) {
                  const double hi = fmax(top[jj][i], x), lo = fmin(top[jj][i], x);
                  top[jj][i] = hi;
                  x = lo;
                }
              }
            }
            if (mode != STAT_TOP) {
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                double x = sc[i];
#pragma unroll
                for (int jj = 0; jj < D; ++jj) {
                  const double lo = fmin(bot[jj][i], x), hi = fmax(bot[jj][i], x);
                  bot[jj][i] = lo;
                  x = hi;
                }
              }
            }
            if (s >= first && s + 1 < ns) {  // wave-uniform; the quorum only
              bool alive = false;
              if (mode == STAT_BOT) {
#pragma unroll
                for (int i = 0; i < 4; ++i) alive |= !(bot[D - 1][i] < cut);  // +inf until D slots are in
              } else {
                const int short_of = D - (ns - 1 - s);  // >= 1 from slot ns - D on
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                  int n = 0;
#pragma unroll
                  for (int jj = 0; jj < D; ++jj) n += top[jj][i] >= cut;
                  alive |= n >= short_of;
                }
              }
              if (!__ballot(alive)) {
                live = false;
                break;
              }
            }
          }
          if (!live) continue;  // no element of the tile reaches cut
          const d4v res = mode == STAT_TOP ? top[D - 1] : mode == STAT_BOT ? bot[D - 1] : top[D - 1] - bot[D - 1];
          if (!A.select) {
            asm volatile("" ::"v"(res[0]), "v"(res[1]), "v"(res[2]), "v"(res[3]));  // keep the score phase live
            continue;
          }
          // first the value alone against the larger of the two bounds (equal values stay in: the
          // key decides below); nearly every tile ends here once the buffer holds N
          if (!__ballot(res[0] >= cut || res[1] >= cut || res[2] >= cut || res[3] >= cut)) continue;
          bool pass[4];
          long long key[4];
          unsigned long long mk[4];
          int n = 0;
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int b = b0 + kk + 4 * i;
            // the triple's packed key, q in its sorted place
            key[i] = b > q ? ((long long)q * PP + b) * PP + c
                   : c > q ? ((long long)b * PP + q) * PP + c
                           : ((long long)b * PP + c) * PP + q;
            pass[i] = b < c && c < P && b != q && c != q && !(res[i] < gthr) &&
                      before(res[i], key[i], thr_s, thr_k);
            pass[i] = pass[i] && !((blk >> i) & 1u);
            if (pass[i] && khi > klo) pass[i] = !is_known(A.known, klo, khi, (long long)b * PP + c);
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
              cs[at] = res[i];
              ck[at] = key[i];
            }
            pos += __popcll(mk[i]);
          }
        }
      }
      __syncthreads();
      if (!st->overflow) break;
      wg_keep_best(st, cs, ck, A.N, shared);
    }
  }
  wg_keep_best(st, cs, ck, A.N, shared);
  const int cnt = st->count;
  for (int i = threadIdx.x; i < cnt; i += NT) {
    A.list_s[(size_t)blockIdx.x * A.N + i] = cs[i];
    A.list_k[(size_t)blockIdx.x * A.N + i] = ck[i];
  }
  if (threadIdx.x == 0) A.list_n[blockIdx.x] = cnt;
}

// ------------------------------------------------------------------------------------------
// Merge, grid (lists out per query, Q): workgroup (w, i) keeps the best N of query i's lists
// [FAN w, FAN (w + 1)); the last level (one workgroup per query) writes the query's row: scores,
// gene ids in key order, count, NaN / -1 tail.
// ------------------------------------------------------------------------------------------
struct PMergeArgs {
  const double* in_s;   // [Q][n_in][N]
  const long long* in_k;
  const int* in_n;
  int n_in;             // lists per query
  double* out_s;        // next level's lists [Q][gridDim.x][N] (null on the last level)
  long long* out_k;
  int* out_n;
  const int* order;     // last level
  double* scores;       // [Q][N]
  int* ids;             // [Q][N][3]
  long long* count;     // [Q]
  int N, cap, P;
};

__global__ __launch_bounds__(NT) void partners_merge_kernel(PMergeArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* cs = reinterpret_cast<double*>(smem + sizeof(Sel));
  long long* ck = reinterpret_cast<long long*>(cs + A.cap);
  if (threadIdx.x == 0) sel_init(st);
  __syncthreads();
  const int qi = blockIdx.y;
  const int base = qi * A.n_in, l0 = base + blockIdx.x * FAN, l1 = min(l0 + FAN, base + A.n_in);
  wg_merge_lists(st, cs, ck, A.in_s, A.in_k, A.in_n, l0, l1, A.N, A.cap);
  wg_keep_best(st, cs, ck, A.N, nullptr);
  const int cnt = st->count;
  if (A.out_s) {
    const size_t o = (size_t)qi * gridDim.x + blockIdx.x;
    for (int i = threadIdx.x; i < cnt; i += NT) {
      A.out_s[o * A.N + i] = cs[i];
      A.out_k[o * A.N + i] = ck[i];
    }
    if (threadIdx.x == 0) A.out_n[o] = cnt;
    return;
  }
  const long long PP = A.P;
  double* scores = A.scores + (size_t)qi * A.N;
  int* ids = A.ids + (size_t)qi * A.N * 3;
  for (int i = threadIdx.x; i < A.N; i += NT) {
    if (i < cnt) {
      const long long k = ck[i];
      scores[i] = cs[i];
      ids[3 * i] = A.order[k / (PP * PP)];
      ids[3 * i + 1] = A.order[(k / PP) % PP];
      ids[3 * i + 2] = A.order[k % PP];
    } else {
      scores[i] = __builtin_nan("");
      ids[3 * i] = ids[3 * i + 1] = ids[3 * i + 2] = -1;
    }
  }
  if (threadIdx.x == 0) A.count[qi] = cnt;
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
struct PartPlan {
  ScanShape sh;
  int N, cap, gpq, n1;
  long long Q;
  size_t off_q, off_qpos, off_thT, off_T, off_ls[2], off_lk[2], off_ln[2], total;
};

// Everything that sizes the workspace follows the context's shape, Q and N only (not the sample
// argument), so one workspace serves every call of that shape.
int make_plan(const mmsbm_ctx* c, long long Q, int N, PartPlan* p) {
  ScanShape& sh = p->sh;
  if (int rc = scan_shape(c, "the partner scan", &sh)) return rc;
  if (N < 1) return fail(MMSBM_ERR_INVALID, "N=%d < 1", N);
  if (N > PARTNERS_MAX_N)
    return fail(MMSBM_ERR_UNSUPPORTED, "N=%d above the partner scan's cap of %d", N, PARTNERS_MAX_N);
  if (Q < 0 || Q > 65535) return fail(MMSBM_ERR_INVALID, "Q=%lld outside [0, 65535]", Q);
  if (int rc = packed_keys_fit(sh)) return rc;
  p->N = N;
  p->Q = Q;
  p->cap = 512;
  while (p->cap < 2 * N) p->cap <<= 1;
  // workgroups per query: the device's worth over Q, no more than a query has items at the
  // narrowest row block, at most two merge levels
  const long long Q1 = std::max<long long>(Q, 1);
  const long long items_max = (long long)((sh.P + 15) / 16) * (sh.P16 / 16);
  const long long want = (8LL * std::max(sh.ncu, 1) + Q1 - 1) / Q1;
  p->gpq = (int)std::max<long long>(1, std::min<long long>({want, items_max, (long long)MAX_GPQ}));
  p->n1 = (p->gpq + FAN - 1) / FAN;
  const size_t B = sh.B, K = sh.K, KP = sh.KP, P16 = sh.P16, q = (size_t)Q1;
  size_t off = align256(sizeof(unsigned long long) * q);  // [0, 8 Q): the published thresholds
  p->off_q = off, off = align256(off + sizeof(int) * q);
  p->off_qpos = off, off = align256(off + sizeof(int) * q);
  p->off_thT = off, off = align256(off + sizeof(double) * B * KP * P16);
  p->off_T = off, off = align256(off + sizeof(double) * B * q * 3 * K * KP);
  const size_t nl[2] = {q * p->gpq, q * p->n1};
  for (int i = 0; i < 2; ++i) {
    p->off_ls[i] = off, off = align256(off + sizeof(double) * nl[i] * N);
    p->off_lk[i] = off, off = align256(off + sizeof(long long) * nl[i] * N);
    p->off_ln[i] = off, off = align256(off + sizeof(int) * nl[i]);
  }
  p->total = off;
  return MMSBM_OK;
}

constexpr int STAT_MAX_DEPTH = 4;  // the deepest sorted lists partners_stat_kernel is built for

// f(std::integral_constant<int, D>{}) for D in [1, STAT_MAX_DEPTH]
template <class F>
int dispatch_depth(int d, F&& f) {
  switch (d) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    default: return f(std::integral_constant<int, 4>{});
  }
}

// The (stat, arg) of the stat entry over ns scored slots -> the kernel's list depth and mode, after
// the checks of include/mmsbm.h.
int stat_plan(int stat, int arg, int ns, int* depth, int* mode) {
  if (stat == MMSBM_PARTNERS_STAT_QUORUM) {
    if (arg < 1 || arg > ns)
      return fail(MMSBM_ERR_INVALID, "the partner scan: votes m=%d outside [1, %d], the scored slots", arg, ns);
    const int from_top = arg, from_bot = ns - arg + 1;  // the m-th largest is the (ns - m + 1)-th smallest
    *depth = std::min(from_top, from_bot);
    *mode = from_top <= from_bot ? STAT_TOP : STAT_BOT;
    if (*depth > STAT_MAX_DEPTH)
      return fail(MMSBM_ERR_UNSUPPORTED,
                  "the partner scan: m=%d of %d slots needs a sorted list of depth %d, above the cap of %d "
                  "(mmsbm_partners_stat_max_depth)",
                  arg, ns, *depth, STAT_MAX_DEPTH);
    return MMSBM_OK;
  }
  if (stat == MMSBM_PARTNERS_STAT_SPREAD) {
    if (ns < 2)
      return fail(MMSBM_ERR_INVALID, "the partner scan: %d active slot: one restart has no spread", ns);
    if (arg < 0 || ns - 2 * (long long)arg < 2)
      return fail(MMSBM_ERR_INVALID,
                  "the partner scan: trim=%d outside [0, %d]: %d scored slots must keep two scores", arg,
                  (ns - 2) / 2, ns);
    *depth = arg + 1;
    *mode = STAT_SPREAD;
    if (*depth > STAT_MAX_DEPTH)
      return fail(MMSBM_ERR_UNSUPPORTED,
                  "the partner scan: trim=%d of %d slots needs two sorted lists of depth %d, above the cap of %d "
                  "(mmsbm_partners_stat_max_depth)",
                  arg, ns, *depth, STAT_MAX_DEPTH);
    return MMSBM_OK;
  }
  return fail(MMSBM_ERR_INVALID, "the partner scan: unknown statistic %d", stat);
}

// Every entry point; `masked`: the call reads a pair mask (mmsbm_partners_topn_masked, whose mask must
// not be null, or mmsbm_partners_stat_topn with one).  stat = null: the list of `sample`; otherwise the
// list of the statistic (stat[0], stat[1]) = (stat, arg) over the active slots (partners_stat_kernel),
// with sample = -1.
int partners_call(mmsbm_ctx* c, const int32_t* order, const int32_t* queries_host, int64_t Q,
                  const int64_t* known_off, const int64_t* known_pairs, const uint32_t* mask, bool masked,
                  const double* theta, const double* pr, int32_t sample, const int32_t* stat, int32_t N, void* ws,
                  int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  PartPlan p;
  int rc = make_plan(c, Q, N, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  int MW = 0;
  if (masked && (rc = check_pair_mask(sh, "the partner scan", mask, &MW))) return rc;
  int depth = 0, mode = 0;
  if (stat && (rc = stat_plan(stat[0], stat[1], sh.nact, &depth, &mode))) return rc;
  if (Q == 0) return MMSBM_OK;
  if (!order || !queries_host || !theta || !pr || !out_scores || !out_ids || !out_count)
    return fail(MMSBM_ERR_INVALID, "null pointer");
  if (known_off && !known_pairs) return fail(MMSBM_ERR_INVALID, "known_off without known_pairs");
  for (int64_t i = 0; i < Q; ++i)
    if (queries_host[i] < 0 || queries_host[i] >= sh.P)
      return fail(MMSBM_ERR_INVALID, "query %lld: gene id %d outside [0, %d)", (long long)i, queries_host[i], sh.P);
  int ns, s0, WB;
  size_t w_bytes;  // U and L: two W rows per row b; the known pairs are per query (checked above)
  if ((rc = check_call(sh, "the partner scan", "mmsbm_partners_workspace_bytes", nullptr, 0, sample, ws, ws_bytes,
                       p.total, &ns, &s0)))
    return rc;
  if ((rc = pick_wb(sh, "the partner scan", 2, ns, W_LDS_MAX, &WB, &w_bytes))) return rc;
  const size_t cand_bytes = (size_t)p.cap * 16;
  // the masked kernel's bit row of the query lies in front of the candidate buffer
  const size_t qrow_bytes = sizeof(unsigned) * (size_t)((MW + 1) & ~1);
  const int lds = (int)(sizeof(Sel) + w_bytes + qrow_bytes + cand_bytes);
  const int merge_lds = (int)(sizeof(Sel) + cand_bytes);
  static_assert(sizeof(Sel) + W_LDS_MAX + PAIR_MASK_MAX_P / 8 + 2 * PARTNERS_MAX_N * 16 <= LDS_MAX,
                "the query's bit row and the buffer stay in LDS");
  const bool select = env_override("MMSBM_PARTNERS_SELECT", 1) != 0;  // measurement: the bare score phase
  // the quorum's early exit from slot ns - m on (ns: never); measurement: MMSBM_PARTNERS_STAT_EARLY=0
  const bool early = stat && stat[0] == MMSBM_PARTNERS_STAT_QUORUM && env_override("MMSBM_PARTNERS_STAT_EARLY", 1) != 0;

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  const int nq = (int)Q;
  int* ln[2] = {(int*)(w + p.off_ln[0]), (int*)(w + p.off_ln[1])};
  double* ls[2] = {(double*)(w + p.off_ls[0]), (double*)(w + p.off_ls[1])};
  long long* lk[2] = {(long long*)(w + p.off_lk[0]), (long long*)(w + p.off_lk[1])};
  int n_lists = 0;  // per query
  if (sh.P >= 3) {
    HIP_TRY(hipMemsetAsync(w, 0, sizeof(unsigned long long) * nq, s));
    HIP_TRY(hipMemcpyAsync(w + p.off_q, queries_host, sizeof(int) * nq, hipMemcpyHostToDevice, s));
    partners_theta_kernel<<<dim3((sh.KP * sh.P16 + NT - 1) / NT, ns), NT, 0, s>>>(
        order, theta, (double*)(w + p.off_thT), sh.K, sh.KP, sh.P, sh.P16, s0);
    HIP_TRY(hipGetLastError());
    partners_prep_kernel<<<dim3(nq, ns), NT, 0, s>>>(order, (const int*)(w + p.off_q), theta, pr,
                                                     (double*)(w + p.off_T), (int*)(w + p.off_qpos), sh.K,
                                                     sh.KP, sh.R, sh.P, nq, s0);
    HIP_TRY(hipGetLastError());
    PartStatArgs as{};
    PartMaskedArgs& am = as;
    PartArgs& a = am;
    am.mask = mask, am.MW = MW;
    a.thT = (const double*)(w + p.off_thT);
    a.T = (const double*)(w + p.off_T);
    a.qpos = (const int*)(w + p.off_qpos);
    a.known_off = (const long long*)known_off;
    a.known = (const long long*)known_pairs;
    a.list_s = ls[0], a.list_k = lk[0], a.list_n = ln[0];
    a.shared = (unsigned long long*)w;
    a.K = sh.K, a.P = sh.P, a.P16 = sh.P16, a.Q = nq, a.ns = ns, a.N = N, a.cap = p.cap, a.WB = WB;
    a.select = select;
    a.gpq = p.gpq;
    const int nbq = (sh.P + 16 * WB - 1) / (16 * WB), nct = sh.P16 / 16;
    a.ncc = std::max(1, std::min(nct, (p.gpq + nbq - 1) / nbq));  // enough items for the query's workgroups
    n_lists = p.gpq;
    const int G = nq * p.gpq;
    as.mode = mode, as.first = early ? ns - stat[1] : ns;
    rc = dispatch_ks(sh.KP / 4, [&](auto ks) {
      constexpr int KS = decltype(ks)::value;
      if (stat)
        return dispatch_depth(depth, [&](auto d) {
          return launch_lds(partners_stat_kernel<KS, decltype(d)::value>, G, lds, s, as);
        });
      if (masked) return launch_lds(partners_masked_kernel<KS>, G, lds, s, am);
      return launch_lds(partners_kernel<KS>, G, lds, s, a);
    });
    if (rc) return rc;
  }
  int cur = 0;
  for (;;) {
    const bool last = n_lists <= FAN;
    PMergeArgs ma{};
    ma.in_s = ls[cur], ma.in_k = lk[cur], ma.in_n = ln[cur], ma.n_in = n_lists;
    if (!last) ma.out_s = ls[cur ^ 1], ma.out_k = lk[cur ^ 1], ma.out_n = ln[cur ^ 1];
    ma.order = order, ma.scores = out_scores, ma.ids = out_ids, ma.count = (long long*)out_count;
    ma.N = N, ma.cap = p.cap, ma.P = std::max(sh.P, 1);
    const int n_out = last ? 1 : (n_lists + FAN - 1) / FAN;
    if ((rc = launch_lds(partners_merge_kernel, dim3(n_out, nq), merge_lds, s, ma))) return rc;
    if (last) break;
    n_lists = n_out;
    cur ^= 1;
  }
  return MMSBM_OK;
}

}  // namespace

extern "C" {

int mmsbm_partners_max_n(void) { return PARTNERS_MAX_N; }

int mmsbm_partners_workspace_bytes(const mmsbm_ctx* c, int64_t Q, int32_t N, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  PartPlan p;
  int rc = make_plan(c, Q, N, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_partners_topn(mmsbm_ctx* c, const int32_t* order, const int32_t* queries_host, int64_t Q,
                        const int64_t* known_off, const int64_t* known_pairs, const double* theta,
                        const double* pr, int32_t sample, int32_t N, void* ws, int64_t ws_bytes,
                        double* out_scores, int32_t* out_ids, int64_t* out_count, void* stream) {
  return partners_call(c, order, queries_host, Q, known_off, known_pairs, nullptr, false, theta, pr, sample, nullptr,
                       N, ws, ws_bytes, out_scores, out_ids, out_count, stream);
}

int mmsbm_partners_topn_masked(mmsbm_ctx* c, const int32_t* order, const int32_t* queries_host, int64_t Q,
                               const int64_t* known_off, const int64_t* known_pairs, const uint32_t* mask,
                               const double* theta, const double* pr, int32_t sample, int32_t N, void* ws,
                               int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count,
                               void* stream) {
  return partners_call(c, order, queries_host, Q, known_off, known_pairs, mask, true, theta, pr, sample, nullptr, N,
                       ws, ws_bytes, out_scores, out_ids, out_count, stream);
}

int mmsbm_partners_stat_max_depth(void) { return STAT_MAX_DEPTH; }

int mmsbm_partners_stat_topn(mmsbm_ctx* c, const int32_t* order, const int32_t* queries_host, int64_t Q,
                             const int64_t* known_off, const int64_t* known_pairs, const uint32_t* mask,
                             const double* theta, const double* pr, int32_t stat, int32_t arg, int32_t N, void* ws,
                             int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count,
                             void* stream) {
  const int32_t stat_arg[2] = {stat, arg};
  return partners_call(c, order, queries_host, Q, known_off, known_pairs, mask, mask != nullptr, theta, pr, -1,
                       stat_arg, N, ws, ws_bytes, out_scores, out_ids, out_count, stream);
}

}  // extern "C"
