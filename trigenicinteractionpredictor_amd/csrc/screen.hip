// screen.hip — MI355X (gfx950) kernels + C ABI (include/mmsbm.h, mmsbm_screen_*) of the screen scan:
// for each query PAIR of genes, the score of every third gene (the pair's predicted interaction
// profile across the array) and the exact top N of them.
//
// Notation as in scan.hip: Th' = theta in rank order (ids sorted by str(id)), p_1 the rating-1
// lattice, a triple three rank positions sorted ascending.  A query is two rank positions x < y, a
// candidate a third position c, and the score of {x, y, c} factors through the two slots the query
// fills:
//   c < x:      S = v1 . Th'[c],  v1[i] = sum_j sum_k p_1[i][j][k] Th'[x][j] Th'[y][k]
//   x < c < y:  S = v2 . Th'[c],  v2[j] = sum_i sum_k p_1[i][j][k] Th'[x][i] Th'[y][k]
//   y < c:      S = v3 . Th'[c],  v3[k] = sum_i sum_j p_1[i][j][k] Th'[x][i] Th'[y][j]
// so Q queries are a [Q][P] GEMM of inner size K whose A row changes with the column's region:
//   v1, v2, v3          about 3 K^3 fma per query and sample   (screen_prep_kernel)
//   S[q][c] = v . Th'[c]                                       (screen_score_kernel, v_mfma_f64_16x16x4)
//   the best N of a row                                        (screen_select_kernel, scan_select.h)
//
// screen_score_kernel: a tile is 16 queries x 16 positions c.  The A operand is the queries' v, read
// from V (tiny, cache-resident: no LDS), the B operand thT.  A tile runs up to three chains (v1, v2,
// v3), each from zero, and every element keeps the chain of its own region; a chain no element of
// the wave's tile needs is skipped (wave-uniform, no bits change).  The ensemble forms each slot's
// tile from zero, adds the tiles in slot order and divides by the slot count (scan_score.h's
// tile_mean rule).  The kernel decides eligibility too and writes NaN at an ineligible place, so
// mmsbm_screen_scores' row and the row mmsbm_screen_topn ranks are the same words.
// screen_select_kernel: one workgroup per query reads the query's row, appends what is not NaN to
// its candidate buffer (wave_reserve, wg_keep_best) and writes the best N: it sees the whole row, so
// there is no merge and no published bound.  Every sum has a fixed order and no score is formed by
// an atomic: a query's row depends on (x, y), the sample and the eligibility only.
// screen_stat_kernel (mmsbm_screen_stat_*): the same tile with an order statistic of the slots' own
// scores in the mean's place, the quorum score q_m or the spread q_{1+t} - q_{ns-t}, from
// per-element sorted lists in registers; the rest of a stat call is the screen scan's host side.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "mmsbm.h"
#include "scan_host.h"
#include "scan_select.h"

namespace {

using namespace scan_host;
using namespace scan_select;

constexpr int SCREEN_MAX_N = 1024;                  // documented cap of N (include/mmsbm.h): the buffer stays in LDS
constexpr size_t ROW_BUDGET = (size_t)256 << 20;    // bytes of score rows one pass may hold
constexpr int SCORE_GRID_X = 4096;                  // most workgroups along c of the score kernel

// ------------------------------------------------------------------------------------------
// Prep
// ------------------------------------------------------------------------------------------
// rank[order[a]] = a over a table preset to -1.  grid ceil(P / NT).
__global__ __launch_bounds__(NT) void screen_rank_kernel(const int* __restrict__ order, int* __restrict__ rank,
                                                         int P) {
  const int a = blockIdx.x * NT + threadIdx.x;
  if (a >= P) return;
  const int g = order[a];
  if (g >= 0 && g < P) rank[g] = a;
}

// Th' k-major and zero-padded: thT[s][KP][P16] (the partner scan's layout).  grid (ceil(KP P16 / NT), samples).
__global__ __launch_bounds__(NT) void screen_theta_kernel(const int* __restrict__ order,
                                                          const double* __restrict__ theta,
                                                          double* __restrict__ thT, int K, int KP, int P, int P16,
                                                          int s0) {
  const int idx = blockIdx.x * NT + threadIdx.x, s = blockIdx.y;
  if (idx >= KP * P16) return;
  const int k = idx / P16, a = idx % P16;
  int g = a < P ? order[a] : -1;
  if (g < 0 || g >= P) g = -1;  // outside the table: a zero row
  thT[(size_t)s * KP * P16 + idx] = (g >= 0 && k < K) ? theta[((size_t)(s0 + s) * P + g) * K + k] : 0.0;
}

// V[s][nq][3][KP] of the pass's queries (zero-padded to KP) and their sorted positions xy[q][2]
// ((-1, -1): the query has no candidate).  The y slot is contracted first, then the x slot, each one
// fma chain over ascending index.  grid (nq, samples); pairs and xy are indexed by the query's place
// in the call.
__global__ __launch_bounds__(NT) void screen_prep_kernel(const int* __restrict__ rank, const int* __restrict__ order,
                                                         const int* __restrict__ pairs,
                                                         const double* __restrict__ theta,
                                                         const double* __restrict__ pr, double* __restrict__ V,
                                                         int* __restrict__ xy, int K, int KP, int R, int P, int nq,
                                                         int q_base, int s0) {
  __shared__ double thx[MMSBM_MAX_K], thy[MMSBM_MAX_K];
  __shared__ double uA[MMSBM_MAX_K * MMSBM_MAX_K];  // uA[i][j] = sum_k p_1[i][j][k] Th'[y][k]
  __shared__ double uB[MMSBM_MAX_K * MMSBM_MAX_K];  // uB[i][k] = sum_j p_1[i][j][k] Th'[y][j]
  const int r = blockIdx.x, s = blockIdx.y;
  const int gq = q_base + r;
  const int ra = rank[pairs[2 * gq]], rb = rank[pairs[2 * gq + 1]];  // ids in [0, P): checked on the host
  int x = min(ra, rb), y = max(ra, rb);
  if (x < 0 || x == y) x = y = -1;  // order is no permutation
  if (s == 0 && threadIdx.x == 0) {
    xy[2 * gq] = x;
    xy[2 * gq + 1] = y;
  }
  double* __restrict__ Vq = V + ((size_t)s * nq + r) * 3 * KP;
  if (x < 0) {
    for (int idx = threadIdx.x; idx < 3 * KP; idx += NT) Vq[idx] = 0.0;
    return;
  }
  const size_t K2 = (size_t)K * K, K3 = K2 * K;
  if ((int)threadIdx.x < K) {
    thx[threadIdx.x] = theta[((size_t)(s0 + s) * P + order[x]) * K + threadIdx.x];
    thy[threadIdx.x] = theta[((size_t)(s0 + s) * P + order[y]) * K + threadIdx.x];
  }
  __syncthreads();
  const double* __restrict__ p1 = pr + ((size_t)(s0 + s) * R + 1) * K3;
  for (int idx = threadIdx.x; idx < 2 * K * K; idx += NT) {
    const int t = idx / (K * K), i = (idx / K) % K, a = idx % K;
    // t = 0: a = j, the chain runs over k (stride 1); t = 1: a = k, the chain runs over j (stride K)
    const double* __restrict__ p = t == 0 ? p1 + i * K2 + (size_t)a * K : p1 + i * K2 + a;
    const size_t step = t == 0 ? (size_t)1 : (size_t)K;
    double v = 0.0;
    for (int n = 0; n < K; ++n) v = fma(p[n * step], thy[n], v);
    (t == 0 ? uA : uB)[i * K + a] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < 3 * KP; idx += NT) {
    const int reg = idx / KP, a = idx % KP;
    double v = 0.0;
    if (a < K) {
      if (reg == 0) {  // v1[i] = sum_j uA[i][j] Th'[x][j]
        for (int j = 0; j < K; ++j) v = fma(uA[a * K + j], thx[j], v);
      } else {         // v2[j] = sum_i uA[i][j] Th'[x][i],  v3[k] = sum_i uB[i][k] Th'[x][i]
        const double* u = reg == 1 ? uA : uB;
        for (int i = 0; i < K; ++i) v = fma(u[i * K + a], thx[i], v);
      }
    }
    Vq[idx] = v;
  }
}

// ------------------------------------------------------------------------------------------
// Score
// ------------------------------------------------------------------------------------------
struct ScreenArgs {
  const double* thT;           // [ns][KP][P16]
  const double* V;             // [ns][nq][3][KP]
  const int* xy;               // [Q][2] sorted rank positions of every query of the call
  const long long* known_off;  // [Q + 1] (null: no exclusion)
  const int* known;            // each query's sorted third positions
  const unsigned* mask;        // [P16][MW] (null: none)
  double* out;                 // row r of the pass at out + r ld
  long long ld;
  int K, P, P16, MW, ns, nq, q_base;
};

__device__ __forceinline__ bool blocked(const unsigned* __restrict__ mask, int MW, int a, int b) {  // a < b < P
  return (mask[(size_t)a * MW + (b >> 5)] >> (b & 31)) & 1u;
}

__device__ __forceinline__ bool third_known(const int* __restrict__ known, long long lo, const long long end, int c) {
  long long hi = end;
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (known[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  return lo < end && known[lo] == c;
}

// grid (c-tile groups, query tiles of 16).  Wave w of workgroup bx takes the c-tiles 4 bx + w,
// 4 (bx + gridDim.x) + w, ...
template <int KS>
__global__ __launch_bounds__(NT) void screen_score_kernel(ScreenArgs A) {
  constexpr int KP = 4 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int P = A.P, P16 = A.P16, ns = A.ns, nq = A.nq;
  const int q0 = blockIdx.y * 16;
  const int arow = min(q0 + m, nq - 1);  // rows past the pass repeat its last query; they are not written
  // the lane's four output rows q0 + kk + 4 i: positions, known slice, the query's own pair
  int xs[4], ys[4];
  long long klo[4], khi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = q0 + kk + 4 * i;
    xs[i] = ys[i] = -1;
    klo[i] = khi[i] = 0;
    if (r < nq) {
      const int gq = A.q_base + r;
      xs[i] = A.xy[2 * gq];
      ys[i] = A.xy[2 * gq + 1];
      if (A.known_off) {
        klo[i] = A.known_off[gq];
        khi[i] = A.known_off[gq + 1];
      }
      if (xs[i] >= 0 && A.mask && blocked(A.mask, A.MW, xs[i], ys[i])) xs[i] = ys[i] = -1;  // no candidate
    }
  }
  double areg[3][KS];  // single sample: the A operands live in registers for every tile of the wave
  if (ns == 1) {
#pragma unroll
    for (int reg = 0; reg < 3; ++reg)
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) areg[reg][ks] = A.V[((size_t)arow * 3 + reg) * KP + 4 * ks + kk];
  }
  const int nct = P16 / 16;
  const double div = (double)ns;
  for (int ct = blockIdx.x * 4 + wave; ct < nct; ct += gridDim.x * 4) {
    const int c = ct * 16 + m;  // < P16
    int region[4];
    bool mine[3] = {false, false, false};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      region[i] = c < xs[i] ? 0 : c < ys[i] ? 1 : 2;
      if (xs[i] >= 0 && c < P) {
        mine[0] |= region[i] == 0;
        mine[1] |= region[i] == 1;
        mine[2] |= region[i] == 2;
      }
    }
    const bool need[3] = {__ballot(mine[0]) != 0, __ballot(mine[1]) != 0, __ballot(mine[2]) != 0};  // wave-uniform
    d4v tot = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < ns; ++s) {
      const double* __restrict__ tc = A.thT + ((size_t)s * KP + kk) * P16 + c;
      double b[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) b[ks] = tc[(size_t)(4 * ks) * P16];
      d4v res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int reg = 0; reg < 3; ++reg) {
        if (!need[reg]) continue;
        d4v acc = {0.0, 0.0, 0.0, 0.0};
        if (ns == 1) {
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[reg][ks], b[ks], acc, 0, 0, 0);
        } else {
          const double* __restrict__ vr = A.V + (((size_t)s * nq + arow) * 3 + reg) * KP + kk;
#pragma unroll
          for (int ks = 0; ks < KS; ++ks)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vr[4 * ks], b[ks], acc, 0, 0, 0);
        }
        // lane holds S[q0 + kk + 4 i][c]: every element keeps the chain of its own region
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (region[i] == reg) res[i] = acc[i];
      }
      tot = s == 0 ? res : tot + res;  // samples added in slot order
    }
    if (ns > 1) tot = tot / div;
    if (c >= P) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = q0 + kk + 4 * i;
      if (r >= nq) continue;
      const int x = xs[i], y = ys[i];
      bool ok = x >= 0 && c != x && c != y;
      if (ok && khi[i] > klo[i]) ok = !third_known(A.known, klo[i], khi[i], c);
      if (ok && A.mask) ok = !blocked(A.mask, A.MW, min(x, c), max(x, c)) && !blocked(A.mask, A.MW, min(y, c), max(y, c));
      A.out[(size_t)r * A.ld + c] = ok ? tot[i] : __builtin_nan("");
    }
  }
}

// ------------------------------------------------------------------------------------------
// Stat score: the row of a statistic of the slots' own scores (mmsbm_screen_stat_*).  The tiling, the
// grid, the wave-to-c-tile rule, the region ballots, the eligibility and the store tail are
// screen_score_kernel's.  Each slot's `res` is formed as that kernel's ensemble path forms it (A from
// V[s][q][reg][KP], B from thT, every needed region's chain from zero), so it is the word
// mmsbm_screen_scores(sample = s) writes; instead of being added to a total it is inserted into two
// per-element sorted lists of depth D held in registers, `top` (the D largest, descending) and `bot`
// (the D smallest, ascending), by the max / min chain of scan_score.h's tile_spread with
// compile-time indices.  The wave-uniform `mode` picks the value once the row's slots are all in
// (nothing is selected before the row is complete, so no slot is skipped): the D-th largest, the
// D-th smallest or their difference, one IEEE subtraction.  The host guarantees D <= ns (quorum) or
// 2 D <= ns (spread), so no start value reaches the output.  No floating-point value is combined
// across slots except in that subtraction.
// ------------------------------------------------------------------------------------------
enum : int { STAT_TOP = 0, STAT_BOT = 1, STAT_SPREAD = 2 };

template <int KS, int D>
__global__ __launch_bounds__(NT) void screen_stat_kernel(ScreenArgs A, int mode) {
  constexpr int KP = 4 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int P = A.P, P16 = A.P16, ns = A.ns, nq = A.nq;
  const int q0 = blockIdx.y * 16;
  const int arow = min(q0 + m, nq - 1);  // rows past the pass repeat its last query; they are not written
  // the lane's four output rows q0 + kk + 4 i: positions, known slice, the query's own pair
  int xs[4], ys[4];
  long long klo[4], khi[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int r = q0 + kk + 4 * i;
    xs[i] = ys[i] = -1;
    klo[i] = khi[i] = 0;
    if (r < nq) {
      const int gq = A.q_base + r;
      xs[i] = A.xy[2 * gq];
      ys[i] = A.xy[2 * gq + 1];
      if (A.known_off) {
        klo[i] = A.known_off[gq];
        khi[i] = A.known_off[gq + 1];
      }
      if (xs[i] >= 0 && A.mask && blocked(A.mask, A.MW, xs[i], ys[i])) xs[i] = ys[i] = -1;  // no candidate
    }
  }
  const int nct = P16 / 16;
  const double inf = __builtin_huge_val();
  for (int ct = blockIdx.x * 4 + wave; ct < nct; ct += gridDim.x * 4) {
    const int c = ct * 16 + m;  // < P16
    int region[4];
    bool mine[3] = {false, false, false};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      region[i] = c < xs[i] ? 0 : c < ys[i] ? 1 : 2;
      if (xs[i] >= 0 && c < P) {
        mine[0] |= region[i] == 0;
        mine[1] |= region[i] == 1;
        mine[2] |= region[i] == 2;
      }
    }
    const bool need[3] = {__ballot(mine[0]) != 0, __ballot(mine[1]) != 0, __ballot(mine[2]) != 0};  // wave-uniform
    d4v top[D], bot[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      top[j] = d4v{-inf, -inf, -inf, -inf};
      bot[j] = d4v{inf, inf, inf, inf};
    }
    for (int s = 0; s < ns; ++s) {
      const double* __restrict__ tc = A.thT + ((size_t)s * KP + kk) * P16 + c;
      double b[KS];
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) b[ks] = tc[(size_t)(4 * ks) * P16];
      d4v res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int reg = 0; reg < 3; ++reg) {
        if (!need[reg]) continue;
        d4v acc = {0.0, 0.0, 0.0, 0.0};
        const double* __restrict__ vr = A.V + (((size_t)s * nq + arow) * 3 + reg) * KP + kk;
#pragma unroll
        for (int ks = 0; ks < KS; ++ks)
          acc = __builtin_amdgcn_mfma_f64_16x16x4f64(vr[4 * ks], b[ks], acc, 0, 0, 0);
        // lane holds S[q0 + kk + 4 i][c]: every element keeps the chain of its own region
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (region[i] == reg) res[i] = acc[i];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double x = res[i], y = res[i];
#pragma unroll
        for (int j = 0; j < D; ++j) {  // each list keeps the better of the two, x / y carry the other on
          const double hi = fmax(top[j][i], x), lo = fmin(top[j][i], x);
          top[j][i] = hi;
          x = lo;
          const double lo2 = fmin(bot[j][i], y), hi2 = fmax(bot[j][i], y);
          bot[j][i] = lo2;
          y = hi2;
        }
      }
    }
    const d4v tot = mode == STAT_TOP ? top[D - 1] : mode == STAT_BOT ? bot[D - 1] : top[D - 1] - bot[D - 1];
    if (c >= P) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = q0 + kk + 4 * i;
      if (r >= nq) continue;
      const int x = xs[i], y = ys[i];
      bool ok = x >= 0 && c != x && c != y;
      if (ok && khi[i] > klo[i]) ok = !third_known(A.known, klo[i], khi[i], c);
      if (ok && A.mask) ok = !blocked(A.mask, A.MW, min(x, c), max(x, c)) && !blocked(A.mask, A.MW, min(y, c), max(y, c));
      A.out[(size_t)r * A.ld + c] = ok ? tot[i] : __builtin_nan("");
    }
  }
}

// ------------------------------------------------------------------------------------------
// Select, grid nq: workgroup r keeps the best N of row r (NaN: not eligible) under the scan's total
// order and writes the query's list: scores, gene ids in key order, count, NaN / -1 tail.
// ------------------------------------------------------------------------------------------
struct SelectArgs {
  const double* rows;  // [nq][ld]
  long long ld;
  const int* xy;       // [Q][2]
  const int* order;
  double* scores;      // [Q][N]
  int* ids;            // [Q][N][3]
  long long* count;    // [Q]
  int N, cap, P, q_base;
};

__global__ __launch_bounds__(NT) void screen_select_kernel(SelectArgs A) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Sel* st = reinterpret_cast<Sel*>(smem);
  double* cs = reinterpret_cast<double*>(smem + sizeof(Sel));
  long long* ck = reinterpret_cast<long long*>(cs + A.cap);
  if (threadIdx.x == 0) sel_init(st);
  __syncthreads();
  const int gq = A.q_base + blockIdx.x, lane = threadIdx.x & 63;
  const int x = A.xy[2 * gq], y = A.xy[2 * gq + 1];
  const long long PP = A.P;
  const double* __restrict__ row = A.rows + (size_t)blockIdx.x * A.ld;
  for (int base = 0; base < A.P; base += NT) {  // every thread runs every round: the barriers below
    const int c = base + threadIdx.x;
    double s = 0.0;
    long long k = 0;
    bool pass = false;
    if (c < A.P && x >= 0) {
      s = row[c];
      // the triple's packed key, c in its sorted place: it rises with c across the three regions
      k = c < x ? ((long long)c * PP + x) * PP + y : c < y ? ((long long)x * PP + c) * PP + y
                                                           : ((long long)x * PP + y) * PP + c;
      pass = s == s && before(s, k, *(volatile double*)&st->thr_s, *(volatile long long*)&st->thr_k);
    }
    bool done = false;
    for (;;) {
      if (!done) {
        const unsigned long long mk = __ballot(pass);
        const int n = __popcll(mk);
        int pos = n ? wave_reserve(st, n, A.cap) : 0;
        if (pos >= 0) {
          if (pass) {
            pos += __popcll(mk & ((1ull << lane) - 1ull));
            cs[pos] = s;
            ck[pos] = k;
          }
          done = true;
        }
      }
      __syncthreads();
      const int full = st->overflow;
      __syncthreads();  // everyone has read the flag before the next round can raise it
      if (!full) break;
      wg_keep_best(st, cs, ck, A.N, nullptr);
    }
  }
  wg_keep_best(st, cs, ck, A.N, nullptr);
  const int cnt = st->count;
  double* scores = A.scores + (size_t)gq * A.N;
  int* ids = A.ids + (size_t)gq * A.N * 3;
  for (int i = threadIdx.x; i < A.N; i += NT) {
    if (i < cnt) {
      const long long key = ck[i];
      scores[i] = cs[i];
      ids[3 * i] = A.order[key / (PP * PP)];
      ids[3 * i + 1] = A.order[(key / PP) % PP];
      ids[3 * i + 2] = A.order[key % PP];
    } else {
      scores[i] = __builtin_nan("");
      ids[3 * i] = ids[3 * i + 1] = ids[3 * i + 2] = -1;
    }
  }
  if (threadIdx.x == 0) A.count[gq] = cnt;
}

// ------------------------------------------------------------------------------------------
// Host side
// ------------------------------------------------------------------------------------------
struct ScreenPlan {
  ScanShape sh;
  int N, cap, C;  // C: queries per pass
  long long Q;
  size_t off_pairs, off_xy, off_rank, off_thT, off_V, off_rows, total;
};

// Everything that sizes the workspace follows the context's shape, Q and N only (not the sample, the
// mask or the pass size, which can only shrink), so one workspace serves every call of that shape.
// N = 0: the plan of mmsbm_screen_scores, which holds no rows.
int make_plan(const mmsbm_ctx* c, long long Q, int N, bool masked, ScreenPlan* p) {
  ScanShape& sh = p->sh;
  mmsbm_detail_scan_shape(c, &sh.device, &sh.K, &sh.R, &sh.B, &sh.P, &sh.nact, &sh.ncu);
  if (sh.K < 1 || sh.K > MMSBM_MAX_K)
    return fail(MMSBM_ERR_UNSUPPORTED, "K=%d outside [1, %d]: call mmsbm_set_shape", sh.K, MMSBM_MAX_K);
  if (sh.R < 2) return fail(MMSBM_ERR_UNSUPPORTED, "the screen scan needs R >= 2 (mmsbm_set_shape)");
  if (sh.B < 1 || sh.P < 0) return fail(MMSBM_ERR_INVALID, "the screen scan needs B >= 1 (mmsbm_set_shape)");
  sh.KP = (sh.K + 3) / 4 * 4;
  sh.P16 = std::max(16, (sh.P + 15) / 16 * 16);
  if (N < 0 || N > SCREEN_MAX_N)
    return fail(MMSBM_ERR_UNSUPPORTED, "N=%d outside the screen scan's [1, %d]", N, SCREEN_MAX_N);
  if (Q < 0 || Q > 65535) return fail(MMSBM_ERR_INVALID, "Q=%lld outside [0, 65535]", Q);
  if (int rc = packed_keys_fit(sh)) return rc;
  int MW;
  if (masked)
    if (int rc = pair_mask_words(sh, "the screen scan", &MW)) return rc;
  p->N = N;
  p->Q = Q;
  p->cap = 512;
  while (p->cap < 2 * N) p->cap <<= 1;
  const size_t B = sh.B, KP = sh.KP, P16 = sh.P16, q = (size_t)std::max<long long>(Q, 1);
  p->C = (int)std::min<size_t>(q, std::max<size_t>(16, ROW_BUDGET / (sizeof(double) * P16)));
  size_t off = 0;
  p->off_pairs = off, off = align256(off + sizeof(int) * 2 * q);
  p->off_xy = off, off = align256(off + sizeof(int) * 2 * q);
  p->off_rank = off, off = align256(off + sizeof(int) * std::max(sh.P, 1));
  p->off_thT = off, off = align256(off + sizeof(double) * B * KP * P16);
  p->off_V = off, off = align256(off + sizeof(double) * B * p->C * 3 * KP);
  p->off_rows = off;
  if (N > 0) off = align256(off + sizeof(double) * p->C * P16);
  p->total = off;
  return MMSBM_OK;
}

constexpr int STAT_MAX_DEPTH = 4;  // the deepest sorted lists screen_stat_kernel is built for

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

// The (stat, arg) of a stat entry over ns scored slots -> the kernel's list depth and mode, after the
// checks of include/mmsbm.h.
int stat_plan(int stat, int arg, int ns, int* depth, int* mode) {
  if (stat == MMSBM_SCREEN_STAT_QUORUM) {
    if (arg < 1 || arg > ns)
      return fail(MMSBM_ERR_INVALID, "the screen scan: votes m=%d outside [1, %d], the scored slots", arg, ns);
    const int from_top = arg, from_bot = ns - arg + 1;  // the m-th largest is the (ns - m + 1)-th smallest
    *depth = std::min(from_top, from_bot);
    *mode = from_top <= from_bot ? STAT_TOP : STAT_BOT;
    if (*depth > STAT_MAX_DEPTH)
      return fail(MMSBM_ERR_UNSUPPORTED,
                  "the screen scan: m=%d of %d slots needs a sorted list of depth %d, above the cap of %d "
                  "(mmsbm_screen_stat_max_depth)",
                  arg, ns, *depth, STAT_MAX_DEPTH);
    return MMSBM_OK;
  }
  if (stat == MMSBM_SCREEN_STAT_SPREAD) {
    if (ns < 2)
      return fail(MMSBM_ERR_INVALID, "the screen scan: %d active slot: one restart has no spread", ns);
    if (arg < 0 || ns - 2 * (long long)arg < 2)
      return fail(MMSBM_ERR_INVALID, "the screen scan: trim=%d outside [0, %d]: %d scored slots must keep two scores",
                  arg, (ns - 2) / 2, ns);
    *depth = arg + 1;
    *mode = STAT_SPREAD;
    if (*depth > STAT_MAX_DEPTH)
      return fail(MMSBM_ERR_UNSUPPORTED,
                  "the screen scan: trim=%d of %d slots needs two sorted lists of depth %d, above the cap of %d "
                  "(mmsbm_screen_stat_max_depth)",
                  arg, ns, *depth, STAT_MAX_DEPTH);
    return MMSBM_OK;
  }
  return fail(MMSBM_ERR_INVALID, "the screen scan: unknown statistic %d", stat);
}

// One call of any entry: N = 0 writes the rows to out_rows [Q][P], N >= 1 the lists.  stat = null:
// the row of `sample` (screen_score_kernel); otherwise the row of the statistic (stat[0], stat[1]) =
// (stat, arg) over the active slots (screen_stat_kernel), with sample = -1.
int screen_run(mmsbm_ctx* c, const int32_t* order, const int32_t* pairs_host, int64_t Q, const int64_t* known_off,
               const int32_t* known_thirds, const uint32_t* mask, const double* theta, const double* pr,
               int32_t sample, const int32_t* stat, int32_t N, void* ws, int64_t ws_bytes, double* out_rows,
               double* out_scores, int32_t* out_ids, int64_t* out_count, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  ScreenPlan p;
  int rc = make_plan(c, Q, N, mask != nullptr, &p);
  if (rc) return rc;
  const ScanShape& sh = p.sh;
  int depth = 0, mode = 0;
  if (stat && (rc = stat_plan(stat[0], stat[1], sh.nact, &depth, &mode))) return rc;
  if (Q == 0) return MMSBM_OK;
  const bool lists = N > 0;
  const char* remedy = "mmsbm_screen_workspace_bytes";
  if (!order || !theta || !pr || !pairs_host ||
      (lists ? (!out_scores || !out_ids || !out_count) : !out_rows))
    return fail(MMSBM_ERR_INVALID, "null pointer");
  if (known_off && !known_thirds) return fail(MMSBM_ERR_INVALID, "known_off without known_thirds");
  if ((uintptr_t)mask & 3) return fail(MMSBM_ERR_INVALID, "the screen scan: misaligned pair mask");
  for (int64_t i = 0; i < 2 * Q; ++i)
    if (pairs_host[i] < 0 || pairs_host[i] >= sh.P)
      return fail(MMSBM_ERR_INVALID, "query %lld: gene id %d outside [0, %d)", (long long)(i / 2), pairs_host[i],
                  sh.P);
  for (int64_t i = 0; i < Q; ++i)
    if (pairs_host[2 * i] == pairs_host[2 * i + 1])
      return fail(MMSBM_ERR_INVALID, "query %lld: a pair of one gene (%d)", (long long)i, pairs_host[2 * i]);
  int ns, s0;
  if ((rc = check_call(sh, "the screen scan", remedy, nullptr, 0, sample, ws, ws_bytes, p.total, &ns, &s0))) return rc;
  static_assert(sizeof(Sel) + 2 * SCREEN_MAX_N * 16 <= 64 * 1024, "the buffer stays in LDS");
  int C = p.C;  // measurement and the tests of the pass boundary: fewer queries per pass
  const long long want = env_override("MMSBM_SCREEN_CHUNK", 0);
  if (want >= 1) C = (int)std::min<long long>(C, want);

  DeviceGuard g(sh.device);
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  const int nQ = (int)Q, MW = (sh.P16 + 31) / 32;
  int* pairs_d = (int*)(w + p.off_pairs);
  int* xy = (int*)(w + p.off_xy);
  int* rank = (int*)(w + p.off_rank);
  double* thT = (double*)(w + p.off_thT);
  double* V = (double*)(w + p.off_V);
  double* rows = (double*)(w + p.off_rows);
  HIP_TRY(hipMemcpyAsync(pairs_d, pairs_host, sizeof(int) * 2 * nQ, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(rank, 0xff, sizeof(int) * sh.P, s));  // -1
  screen_rank_kernel<<<(sh.P + NT - 1) / NT, NT, 0, s>>>(order, rank, sh.P);
  HIP_TRY(hipGetLastError());
  screen_theta_kernel<<<dim3((sh.KP * sh.P16 + NT - 1) / NT, ns), NT, 0, s>>>(order, theta, thT, sh.K, sh.KP, sh.P,
                                                                              sh.P16, s0);
  HIP_TRY(hipGetLastError());
  const int nct = sh.P16 / 16;
  for (int q_base = 0; q_base < nQ; q_base += C) {
    const int nq = std::min(C, nQ - q_base);
    screen_prep_kernel<<<dim3(nq, ns), NT, 0, s>>>(rank, order, pairs_d, theta, pr, V, xy, sh.K, sh.KP, sh.R, sh.P,
                                                   nq, q_base, s0);
    HIP_TRY(hipGetLastError());
    ScreenArgs a{};
    a.thT = thT, a.V = V, a.xy = xy;
    a.known_off = (const long long*)known_off, a.known = known_thirds;
    a.mask = mask, a.MW = MW;
    a.out = lists ? rows : out_rows + (size_t)q_base * sh.P;
    a.ld = lists ? sh.P16 : sh.P;
    a.K = sh.K, a.P = sh.P, a.P16 = sh.P16, a.ns = ns, a.nq = nq, a.q_base = q_base;
    const dim3 grid(std::min((nct + 3) / 4, SCORE_GRID_X), (nq + 15) / 16);
    rc = dispatch_ks(sh.KP / 4, [&](auto ks) {
      if (!stat) {
        screen_score_kernel<decltype(ks)::value><<<grid, NT, 0, s>>>(a);
        HIP_TRY(hipGetLastError());
        return (int)MMSBM_OK;
      }
      return dispatch_depth(depth, [&](auto d) {
        screen_stat_kernel<decltype(ks)::value, decltype(d)::value><<<grid, NT, 0, s>>>(a, mode);
        HIP_TRY(hipGetLastError());
        return (int)MMSBM_OK;
      });
    });
    if (rc) return rc;
    if (!lists) continue;
    SelectArgs sa{};
    sa.rows = rows, sa.ld = sh.P16, sa.xy = xy, sa.order = order;
    sa.scores = out_scores, sa.ids = out_ids, sa.count = (long long*)out_count;
    sa.N = N, sa.cap = p.cap, sa.P = sh.P, sa.q_base = q_base;
    if ((rc = launch_lds(screen_select_kernel, nq, (int)(sizeof(Sel) + (size_t)p.cap * 16), s, sa))) return rc;
  }
  return MMSBM_OK;
}

}  // namespace

extern "C" {

int mmsbm_screen_max_n(void) { return SCREEN_MAX_N; }

int mmsbm_screen_workspace_bytes(const mmsbm_ctx* c, int64_t Q, int32_t N, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  ScreenPlan p;
  int rc = make_plan(c, Q, N, false, &p);
  if (rc) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

int mmsbm_screen_topn(mmsbm_ctx* c, const int32_t* order, const int32_t* pairs_host, int64_t Q,
                      const int64_t* known_off, const int32_t* known_thirds, const uint32_t* mask,
                      const double* theta, const double* pr, int32_t sample, int32_t N, void* ws, int64_t ws_bytes,
                      double* out_scores, int32_t* out_ids, int64_t* out_count, void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  if (N == 0) return fail(MMSBM_ERR_UNSUPPORTED, "N=0 outside the screen scan's [1, %d]", SCREEN_MAX_N);
  return screen_run(c, order, pairs_host, Q, known_off, known_thirds, mask, theta, pr, sample, nullptr, N, ws,
                    ws_bytes, nullptr, out_scores, out_ids, out_count, stream);
}

int mmsbm_screen_scores(mmsbm_ctx* c, const int32_t* order, const int32_t* pairs_host, int64_t Q,
                        const int64_t* known_off, const int32_t* known_thirds, const uint32_t* mask,
                        const double* theta, const double* pr, int32_t sample, void* ws, int64_t ws_bytes,
                        double* out, void* stream) {
  return screen_run(c, order, pairs_host, Q, known_off, known_thirds, mask, theta, pr, sample, nullptr, 0, ws,
                    ws_bytes, out, nullptr, nullptr, nullptr, stream);
}

int mmsbm_screen_stat_max_depth(void) { return STAT_MAX_DEPTH; }

int mmsbm_screen_stat_topn(mmsbm_ctx* c, const int32_t* order, const int32_t* pairs_host, int64_t Q,
                           const int64_t* known_off, const int32_t* known_thirds, const uint32_t* mask,
                           const double* theta, const double* pr, int32_t stat, int32_t arg, int32_t N, void* ws,
                           int64_t ws_bytes, double* out_scores, int32_t* out_ids, int64_t* out_count,
                           void* stream) {
  if (!c) return fail(MMSBM_ERR_INVALID, "null context");
  if (N == 0) return fail(MMSBM_ERR_UNSUPPORTED, "N=0 outside the screen scan's [1, %d]", SCREEN_MAX_N);
  const int32_t stat_arg[2] = {stat, arg};
  return screen_run(c, order, pairs_host, Q, known_off, known_thirds, mask, theta, pr, -1, stat_arg, N, ws, ws_bytes,
                    nullptr, out_scores, out_ids, out_count, stream);
}

int mmsbm_screen_stat_scores(mmsbm_ctx* c, const int32_t* order, const int32_t* pairs_host, int64_t Q,
                             const int64_t* known_off, const int32_t* known_thirds, const uint32_t* mask,
                             const double* theta, const double* pr, int32_t stat, int32_t arg, void* ws,
                             int64_t ws_bytes, double* out, void* stream) {
  const int32_t stat_arg[2] = {stat, arg};
  return screen_run(c, order, pairs_host, Q, known_off, known_thirds, mask, theta, pr, -1, stat_arg, 0, ws, ws_bytes,
                    out, nullptr, nullptr, nullptr, stream);
}

}  // extern "C"
