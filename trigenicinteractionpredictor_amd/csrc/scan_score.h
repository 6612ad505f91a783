// scan_score.h — the score phase shared by the genome-wide scan (scan.hip) and the triangle sweep
// of the score census and the pair census (scan_sweep.h): the prep kernel (Th' k-major, T_a of every
// gene), a work item's W rows in LDS, the MFMA chain of one 16 x 16 tile and the ensemble's
// slot-order sum and division.  Every kernel forms a score through these functions and nothing
// else, so a triple's score carries the same bits in each: the census at the scores of a scan list
// returns each entry's position in that list.
//
// Notation (scan.hip): Th' = theta in rank order, T_a[y][z] = sum_x Th'[a][x] p_1[x][y][z],
// W_a[b][z] = sum_y Th'[b][y] T_a[y][z], S_a[b][c] = sum_z W_a[b][z] Th'[c][z].  A work item is
// (a, a block of 16 WB rows b); wave w of the 4 holds b-tile w % WB and the c-tiles w / WB + i 4 / WB.
#ifndef MMSBM_SCAN_SCORE_H
#define MMSBM_SCAN_SCORE_H

#include "mmsbm.h"
#include "scan_select.h"

namespace scan_score {

using scan_select::d4v;
using scan_select::NT;

constexpr int W_LDS_MAX = 64 * 1024;  // the W rows of one item, every sample (scan_host::pick_wb)

// ------------------------------------------------------------------------------------------
// Prep: Th' k-major and zero-padded (thT[s][KP][P16]) and T_a (T[s][P][K][KP]) of every gene.
// grid (P16, samples).
// ------------------------------------------------------------------------------------------
static __global__ __launch_bounds__(NT) void scan_prep_kernel(const int* __restrict__ order,
                                                              const double* __restrict__ theta,
                                                              const double* __restrict__ pr,
                                                              double* __restrict__ thT, double* __restrict__ T,
                                                              int K, int KP, int R, int P, int P16, int s0) {
  __shared__ double th[MMSBM_MAX_K];
  const int a = blockIdx.x, s = blockIdx.y;
  const size_t K2 = (size_t)K * K, K3 = K2 * K;
  int g = a < P ? order[a] : -1;
  if (g < 0 || g >= P) g = -1;  // outside the table: a zero row (the binding checks the permutation)
  const double* __restrict__ row = theta + ((size_t)(s0 + s) * P + (g < 0 ? 0 : g)) * K;
  if (threadIdx.x < KP) {
    const double v = (g >= 0 && (int)threadIdx.x < K) ? row[threadIdx.x] : 0.0;
    if ((int)threadIdx.x < K) th[threadIdx.x] = v;
    thT[((size_t)s * KP + threadIdx.x) * P16 + a] = v;
  }
  __syncthreads();
  if (a >= P) return;
  const double* __restrict__ p1 = pr + ((size_t)(s0 + s) * R + 1) * K3;
  double* __restrict__ Ta = T + ((size_t)s * P + a) * K * KP;
  for (int idx = threadIdx.x; idx < K * KP; idx += NT) {
    const int y = idx / KP, z = idx % KP;
    double v = 0.0;
    if (z < K)
      for (int x = 0; x < K; ++x) v = fma(th[x], p1[x * K2 + y * K + z], v);
    Ta[idx] = v;
  }
}

template <int KS>
struct Score {
  static constexpr int KP = 4 * KS, WS = KP + 2;  // W row stride: conflict-free A-operand reads

  // W_a of the item's RB rows from bq RB on, every sample (the whole workgroup; barriers are the caller's)
  static __device__ __forceinline__ void fill_w(double* W, const double* __restrict__ Tall,
                                                const double* __restrict__ thT, int a, int bq, int RB,
                                                int ns, int K, int P, int P16) {
    for (int idx = threadIdx.x; idx < ns * RB * KP; idx += NT) {
      const int z = idx % KP, r = (idx / KP) % RB, s = idx / (KP * RB);
      const int rowb = bq * RB + r;
      double v = 0.0;
      if (rowb < P) {
        const double* __restrict__ Ta = Tall + ((size_t)s * P + a) * K * KP + z;
        const double* __restrict__ tb = thT + (size_t)s * KP * P16 + rowb;
        for (int y = 0; y < K; ++y) v = fma(tb[(size_t)y * P16], Ta[y * KP], v);
      }
      W[((size_t)s * RB + r) * WS + z] = v;
    }
  }

  // single sample: the wave's A operand (rows of b-tile wb) stays in registers for the whole item
  static __device__ __forceinline__ void load_a(double (&areg)[KS], const double* W, int wb, int m, int kk) {
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) areg[ks] = W[(size_t)(wb * 16 + m) * WS + 4 * ks + kk];
  }

  // single sample: the Th' operand of the c-tile whose first column is c0
  static __device__ __forceinline__ void load_b(double (&b)[KS], const double* __restrict__ thT, int P16,
                                                int c0, int m, int kk) {
    const double* __restrict__ tc = thT + (size_t)kk * P16 + c0 + m;
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) b[ks] = tc[(size_t)(4 * ks) * P16];
  }

  // lane holds S[b0 + kk + 4 i][c0 + m] in element i
  static __device__ __forceinline__ d4v tile_one(const double (&areg)[KS], const double (&b)[KS]) {
    d4v tot = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) tot = __builtin_amdgcn_mfma_f64_16x16x4f64(areg[ks], b[ks], tot, 0, 0, 0);
    return tot;
  }

  // the ensemble: each sample's tile accumulated from zero, the tiles added in slot order, then
  // divided by the sample count
  static __device__ __forceinline__ d4v tile_mean(const double* W, const double* __restrict__ thT, int ns,
                                                  int RB, int P16, int wb, int c0, int m, int kk, double div) {
    d4v tot = {0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < ns; ++s) {
      const double* __restrict__ tc = thT + ((size_t)s * KP + kk) * P16 + c0 + m;
      const double* wr = W + ((size_t)s * RB + wb * 16 + m) * WS + kk;
      d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], tc[(size_t)(4 * ks) * P16], acc, 0, 0, 0);
      tot = s == 0 ? acc : tot + acc;  // samples added in slot order
    }
    return tot / div;
  }

  // The vote scan (scan_votes.hip): which of a slot's four scores are at or above thr, one byte per
  // element (byte i: element i), so that the bytes of up to 255 slots add without a carry between
  // them (the W tile holds at most 85: 64 KiB / (16 rows of 6 doubles)).
  static __device__ __forceinline__ unsigned votes_of(const d4v& acc, double thr) {
    unsigned v = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) v |= (unsigned)(acc[i] >= thr) << (8 * i);
    return v;
  }

  // tile_mean that also votes: the same operands in the same order, each slot's accumulator compared
  // with thr before it joins the slot-order sum (the accumulator is that slot's single-sample score,
  // bit for bit: tile_one's chain over the same W row and Th' column).  votes: byte i = the slots
  // with element i at or above thr.
  static __device__ __forceinline__ d4v tile_votes(const double* W, const double* __restrict__ thT, int ns,
                                                   int RB, int P16, int wb, int c0, int m, int kk, double div,
                                                   double thr, unsigned& votes) {
    d4v tot = {0.0, 0.0, 0.0, 0.0};
    unsigned v = 0;
    for (int s = 0; s < ns; ++s) {
      const double* __restrict__ tc = thT + ((size_t)s * KP + kk) * P16 + c0 + m;
      const double* wr = W + ((size_t)s * RB + wb * 16 + m) * WS + kk;
      d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], tc[(size_t)(4 * ks) * P16], acc, 0, 0, 0);
      v += votes_of(acc, thr);
      tot = s == 0 ? acc : tot + acc;  // samples added in slot order
    }
    votes = v;
    return tot / div;
  }

  // The quorum scan (scan_quorum.hip): the m-th largest of the slots' own scores, per element.  The
  // same operands in the same order as tile_mean, each slot's accumulator formed from zero (that
  // slot's single-sample score, bit for bit) and inserted into a per-element sorted list of depth D
  // by D max / min pairs with compile-time indices (the list stays in registers).  SMALL = false: the
  // list keeps the D = m largest, descending, and q is the smallest kept.  SMALL = true: it keeps
  // the D = ns - m + 1 smallest, ascending, and q is the largest kept: the m-th largest again.  The
  // caller picks the shorter list; no floating-point value is combined across slots.
  // Early exit.  A triple with q_m < cut is pruned by the selection, and q_m < cut exactly when more
  // than ns - m slots score strictly below cut.  The list already says so: with SMALL its last
  // entry, the (ns - m + 1)-th smallest so far, is below cut exactly then; without, the entries at
  // or above cut plus the slots still to come fall short of m exactly then.  From slot `first` on
  // (the first after which that can hold: ns - m, 0-based; ns or more: never) and before the last
  // slot (after which nothing is saved) one ballot asks whether any element of the wave's tile can
  // still reach cut; if none can, the remaining slots are not formed and the function returns false
  // (wave-uniform).  Equal scores stay in.
  template <int D, bool SMALL>
  static __device__ __forceinline__ bool tile_quorum(const double* W, const double* __restrict__ thT, int ns,
                                                     int RB, int P16, int wb, int c0, int m, int kk, double cut,
                                                     int first, d4v& q) {
    const double start = SMALL ? __builtin_huge_val() : -__builtin_huge_val();
    d4v L[D];
#pragma unroll
    for (int j = 0; j < D; ++j) L[j] = d4v{start, start, start, start};
    for (int s = 0; s < ns; ++s) {
      const double* __restrict__ tc = thT + ((size_t)s * KP + kk) * P16 + c0 + m;
      const double* wr = W + ((size_t)s * RB + wb * 16 + m) * WS + kk;
      d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], tc[(size_t)(4 * ks) * P16], acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double x = acc[i];
#pragma unroll
        for (int j = 0; j < D; ++j) {  // L[j] keeps the better of the two, x carries the other on
          const double lo = fmin(L[j][i], x), hi = fmax(L[j][i], x);
          L[j][i] = SMALL ? lo : hi;
          x = SMALL ? hi : lo;
        }
      }
      if (s >= first && s + 1 < ns) {  // wave-uniform
        bool alive = false;
        if (SMALL) {
#pragma unroll
          for (int i = 0; i < 4; ++i) alive |= !(L[D - 1][i] < cut);  // +inf until D slots are in
        } else {
          const int need = D - (ns - 1 - s);  // >= 1 from slot ns - D on
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            int n = 0;
#pragma unroll
            for (int j = 0; j < D; ++j) n += L[j][i] >= cut;
            alive |= n >= need;
          }
        }
        if (!__ballot(alive)) return false;
      }
    }
    q = L[D - 1];
    return true;
  }

  // The dispute scan (scan_spread.hip): the spread d_t = q_{1+t} - q_{ns-t} of the slots' own scores,
  // per element, for the trim t = D - 1.  The same operands in the same order as tile_mean, each
  // slot's accumulator formed from zero (that slot's single-sample score, bit for bit) and inserted
  // into two per-element sorted lists of depth D, as tile_quorum inserts it into one: `top` keeps the
  // D largest, descending, and `bot` the D smallest, ascending.  The result is one IEEE subtraction,
  // top[D - 1] - bot[D - 1]: the (1 + t)-th largest minus the (1 + t)-th smallest.  The caller
  // guarantees ns >= 2 D, so both entries are slot scores (no start value is left) and the result is
  // >= +0.  Every slot is formed: a spread only grows as slots arrive, so none can be skipped.
  template <int D>
  static __device__ __forceinline__ d4v tile_spread(const double* W, const double* __restrict__ thT, int ns,
                                                    int RB, int P16, int wb, int c0, int m, int kk) {
    const double inf = __builtin_huge_val();
    d4v top[D], bot[D];
#pragma unroll
    for (int j = 0; j < D; ++j) {
      top[j] = d4v{-inf, -inf, -inf, -inf};
      bot[j] = d4v{inf, inf, inf, inf};
    }
    for (int s = 0; s < ns; ++s) {
      const double* __restrict__ tc = thT + ((size_t)s * KP + kk) * P16 + c0 + m;
      const double* wr = W + ((size_t)s * RB + wb * 16 + m) * WS + kk;
      d4v acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int ks = 0; ks < KS; ++ks)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(wr[4 * ks], tc[(size_t)(4 * ks) * P16], acc, 0, 0, 0);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        double x = acc[i], y = acc[i];
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
    return top[D - 1] - bot[D - 1];
  }
};

}  // namespace scan_score

#endif  // MMSBM_SCAN_SCORE_H
