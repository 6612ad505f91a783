// scan_sweep.h — the triangle sweep shared by the score census (census.hip), the pair census
// (pair_census.hip), the threshold scan (scan_above.hip) and the vote scan (scan_votes.hip): every
// eligible triple (the scan's: rank positions a < b < c < P, packed key not among the known ones)
// with its score, handed to the kernel's consumer one 16 x 16 tile at a time.
// The kernels see their triples through sweep() and nothing else, so exactly the same triples are
// hits in either: for every threshold the pair census's counts sum to three times the census's.
//
// The score phase is the scan's (scan_score.h), and so are the work items (a, a block of 16 WB rows
// b), round-robin over the workgroups, and the rule that skips an item.
//
// Exclusion.  Per item two searches bound the known keys whose first two positions fall into the
// item: known[lo, hi).  The workgroup sets one bit per (b-tile, c-tile mod CT_BITS) that holds one
// of them in an LDS bitmap; is_known runs only for the lanes of flagged tiles, over [lo, hi).  A
// c-tile index beyond CT_BITS shares a bit with another: a flag may be set for a tile without known
// keys, which costs searches and nothing else.
#ifndef MMSBM_SCAN_SWEEP_H
#define MMSBM_SCAN_SWEEP_H

#include "scan_score.h"
#include "scan_select.h"

namespace scan_sweep {

using scan_select::d4v;
using scan_select::NT;

constexpr int CT_BITS = 2048;  // c-tile bits per b-tile of the exclusion bitmap
constexpr int BM_WORDS = 4 * CT_BITS / 32;

struct Head {        // the first 64 bytes of the dynamic LDS
  long long lo, hi;  // the item's known keys are known[lo, hi)
  long long pad[6];
};
static_assert(sizeof(Head) == 64, "Head is the first 64 bytes of the dynamic LDS");

struct SweepArgs {
  const double* thT;       // [ns][KP][P16]
  const double* T;         // [ns][P][K][KP]
  const long long* known;  // sorted packed keys (null: none)
  long long n_known;
  int K, P, P16, ns, WB;
};

// Every kernel that sweeps calls this once, after its own LDS fills and before sweep(): the head's
// empty range and the barrier that sweep() starts from.  It is the kernel's call and not sweep()'s
// first statement because, with the store behind sweep()'s own barrier, the compiler no longer reads
// the known keys of the two searches through the scalar cache (1 % of the B = 8 ensemble at K = 10).
__device__ __forceinline__ void sweep_begin(Head* st) {
  if (threadIdx.x == 0) st->lo = st->hi = 0;
  __syncthreads();
}

// The whole workgroup sweeps its items.  The dynamic LDS starts with the head, then W ([ns][16 WB]
// rows of Score<KS>::WS doubles); bm is the kernel's BM_WORDS words for the bitmap.  The kernel has
// called sweep_begin.  ENS: the ensemble (ns > 1; a single sample otherwise).  A template
// parameter, so that neither path holds the other's registers.  A wave that holds rows of an item
// calls begin_item(a, b0) once (the place for what the kernel derives from the item alone, such as
// a row base of its output), which returns the item's consumer; for every tile of the item that
// can hold a triple the wave then calls consume(ct, tot, el): the lane holds
// S_a[b0 + kk + 4 i][16 ct + m] in tot[i] (m = lane & 15, kk = lane >> 4) and el[i] says whether
// that triple is eligible.
//
// VOTES (sweep_votes, for scan_votes.hip): the score phase also compares every scored slot's own
// tile with vthr (Score::tile_votes; a single sample: the one tile) and the consumer is called as
// consume(ct, tot, votes, el), votes holding in byte i the number of slots whose element i is at or
// above vthr, for eligible and other elements alike.  sweep() itself is the instantiation without
// it, which holds nothing of the votes.
//
// MASK (sweep_masked, for the masked census, pair census and threshold scan; sweep_votes_masked with
// VOTES, for the masked vote scan): a triple is eligible only if none of
// its three pairs is set in the pair mask (include/mmsbm.h: mask[P16][MW] in rank positions, bit
// y & 31 of mask[x][y >> 5] blocks the pair x < y).  Per item the workgroup first reads the bits
// (a, the item's rows) through the scalar cache and skips the item when every row b with a < b < P is
// blocked: before the barrier, the known-key searches and fill_w.  Otherwise row a goes to mrow (MW
// words of LDS, the kernel's) with the bitmap, and a lane keeps its four (a, b) bits for the item.
// Per tile the (a, c) bits are halfword ct of mrow: at 0xFFFF the tile's MFMA chain is not issued and
// the consumer is not called (wave-uniform).  The (b, c) bits of a lane's four rows are halfword ct of
// mask rows b0 + kk + 4 i, loaded one tile ahead with the Th' operand.  The lane's blocked elements
// travel with the tile as four bits and are taken out of el after the interior test, which stays as
// it is.  Every index stays inside the mask: rows a < P and b <= b0 + 15 < P16, halfwords ct < P16 / 16
// <= 2 MW.  The instantiations without MASK hold nothing of it.
template <int KS, bool ENS, bool VOTES, bool MASK, class BeginItem>
__device__ __forceinline__ void sweep_impl(const SweepArgs& A, Head* st, double* W, unsigned* bm, double vthr,
                                           [[maybe_unused]] const unsigned* __restrict__ mask,
                                           [[maybe_unused]] int MW, [[maybe_unused]] unsigned* mrow,
                                           BeginItem&& begin_item) {
  using namespace scan_select;
  using Sc = scan_score::Score<KS>;
  const int RB = 16 * A.WB;  // rows b of one item
  const int P = A.P, P16 = A.P16, K = A.K, ns = A.ns;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = lane & 15, kk = lane >> 4;
  const int wb = wave % A.WB, wc = wave / A.WB, CW = 4 / A.WB;
  const int nct = P16 / 16;
  const int nbq = (P + RB - 1) / RB;
  const long long PP = (long long)P;
  const double div = (double)ns;
  const bool has_known = A.n_known > 0;

  // items round-robin over the workgroups, skipped exactly as the scan skips them
  for (long long q = blockIdx.x; q < PP * nbq; q += gridDim.x) {
    const int a = (int)(q / nbq), bq = (int)(q % nbq);
    if (a >= P - 2 || bq * RB + RB - 1 <= a || bq * RB >= P - 1) continue;  // no a < b < c here
    if constexpr (MASK) {
      // the (a, b) bits of the item's rows: RB = 16, 32 or 64 bits from bit bq RB of row a on
      const int r0 = bq * RB, w0 = r0 >> 5;
      const unsigned* __restrict__ ra = mask + (size_t)a * MW;
      unsigned long long bits = (unsigned long long)ra[w0] >> (r0 & 31);  // w0 < MW: r0 < P - 1
      if (RB == 64 && w0 + 1 < MW) bits |= (unsigned long long)ra[w0 + 1] << 32;
      const int lo = max(a + 1, r0) - r0, hi = min(P, r0 + RB) - r0;  // 0 <= lo < hi <= RB, bits inside row a
      const unsigned long long need = (hi >= 64 ? ~0ull : (1ull << hi) - 1) & ~((1ull << lo) - 1);
      if ((bits & need) == need) continue;  // workgroup-uniform: every pair (a, b) of the item is blocked
    }
    __syncthreads();  // the previous item's W, bitmap and range are read
    if constexpr (MASK)
      for (int i = threadIdx.x; i < MW; i += NT) mrow[i] = mask[(size_t)a * MW + i];
    if (has_known) {
      // the known keys whose first position is a and whose second falls into the item's rows
      if (threadIdx.x == 64) st->lo = lower_bound(A.known, 0, A.n_known, ((long long)a * PP + (long long)bq * RB) * PP);
      if (threadIdx.x == 128)
        st->hi = lower_bound(A.known, 0, A.n_known, ((long long)a * PP + (long long)bq * RB + RB) * PP);
      for (int i = threadIdx.x; i < BM_WORDS; i += NT) bm[i] = 0;
    }
    Sc::fill_w(W, A.T, A.thT, a, bq, RB, ns, K, P, P16);  // W_a of the item's rows, every sample
    __syncthreads();
    const long long klo = st->lo, khi = st->hi;
    if (khi > klo) {  // workgroup-uniform
      for (long long i = klo + threadIdx.x; i < khi; i += NT) {
        const long long key = A.known[i];
        const int tb = (int)((key / PP) % PP) / 16 - bq * A.WB, tc = (int)(key % PP) / 16;
        if (tb >= 0 && tb < A.WB)  // always: [klo, khi) holds the item's rows only
          atomicOr(&bm[tb * (CT_BITS / 32) + ((tc & (CT_BITS - 1)) >> 5)], 1u << (tc & 31));
      }
      __syncthreads();
    }

    const int btile = bq * A.WB + wb, b0 = btile * 16;
    const bool wave_on = b0 < P - 1 && b0 + 15 > a;
    if (!wave_on) continue;
    double areg[KS];
    if (!ENS) Sc::load_a(areg, W, wb, m, kk);
    int ct = bq * A.WB + wc;
    while (ct < btile) ct += CW;  // every c of those tiles is below every b
    double bnext[KS];  // single sample: the next tile's Th' operand is in flight
    if (!ENS && ct < nct) Sc::load_b(bnext, A.thT, P16, ct * 16, m, kk);
    auto consume = begin_item(a, b0);
    [[maybe_unused]] unsigned abm = 0;  // bit i: the pair (a, b0 + kk + 4 i) is blocked
    [[maybe_unused]] unsigned bcn[4] = {0, 0, 0, 0};  // the next tile's (b, c) halfwords, in flight
    [[maybe_unused]] const unsigned short* mrow16 = reinterpret_cast<const unsigned short*>(mrow);
    // halfword ct of the lane's four mask rows: one 32-bit lane offset (row b0 + kk; the mask is at
    // most 32 MiB) on four wave-uniform bases, the rows 4 i below it
    [[maybe_unused]] const unsigned bc_off = (unsigned)(b0 + kk) * (unsigned)MW * 4u;
    [[maybe_unused]] auto load_bc = [&](unsigned (&h)[4], int ct) {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        h[i] = *reinterpret_cast<const unsigned short*>(reinterpret_cast<const char*>(mask) + (size_t)(16 * i) * MW +
                                                        (bc_off + 2u * (unsigned)ct));
    };
    if constexpr (MASK) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int b = b0 + kk + 4 * i;
        abm |= ((mrow[b >> 5] >> (b & 31)) & 1u) << i;
      }
      if (ct < nct) load_bc(bcn, ct);
    }
    // Resolve a finished tile's eligibility and hand it over.
    auto finish = [&](const d4v& tot, [[maybe_unused]] unsigned votes, [[maybe_unused]] unsigned blk, int ct) {
      const int c0 = ct * 16, c = c0 + m;
      bool el[4];
      if (b0 > a && c0 > b0 + 15 && c0 + 16 <= P) {  // an interior tile: a < b < c < P everywhere
        el[0] = el[1] = el[2] = el[3] = true;
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int b = b0 + kk + 4 * i;
          el[i] = a < b && b < c && c < P;
        }
      }
      if constexpr (MASK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) el[i] = el[i] && !((blk >> i) & 1u);
      }
      if (khi > klo && ((bm[wb * (CT_BITS / 32) + ((ct & (CT_BITS - 1)) >> 5)] >> (ct & 31)) & 1u)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const long long key = ((long long)a * PP + (b0 + kk + 4 * i)) * PP + c;
          if (el[i]) el[i] = !is_known(A.known, klo, khi, key);
        }
      }
      if constexpr (VOTES)  // a single sample votes with the tile itself: nothing to carry for a tile
        consume(ct, tot, ENS ? votes : Sc::votes_of(tot, vthr), el);
      else
        consume(ct, tot, el);
    };
    // A tile is handed over after the next tile's MFMA chain has been issued, so the consumer's code
    // does not depend on the newest accumulator (measured on the census: 12 % off the B = 8
    // ensemble, nothing at B = 1).
    d4v prev = {0.0, 0.0, 0.0, 0.0};
    int prev_ct = -1;
    [[maybe_unused]] unsigned votes = 0, prev_votes = 0;
    [[maybe_unused]] unsigned blk = 0, prev_blk = 0;  // bit i: element i of the tile is blocked
    for (; ct < nct; ct += CW) {
      const int c0 = ct * 16;
      d4v tot;
      [[maybe_unused]] bool dead = false;  // every pair (a, c) of the tile is blocked (wave-uniform)
      if constexpr (MASK) {
        const unsigned ac = mrow16[ct];
        dead = ac == 0xFFFFu;
        blk = abm | (((ac >> m) & 1u) ? 0xFu : 0u);
#pragma unroll
        for (int i = 0; i < 4; ++i) blk |= ((bcn[i] >> m) & 1u) << i;
        if (ct + CW < nct) load_bc(bcn, ct + CW);
      }
      if (!ENS) {
        double bcur[KS];
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) bcur[ks] = bnext[ks];
        if (ct + CW < nct) Sc::load_b(bnext, A.thT, P16, c0 + 16 * CW, m, kk);
        if constexpr (MASK) {
          if (dead) continue;  // the finished tile waits for the next live one
        }
        tot = Sc::tile_one(areg, bcur);
      } else if constexpr (VOTES) {
        if constexpr (MASK) {
          if (dead) continue;  // before tile_votes: votes and blk stay the finished tile's
        }
        tot = Sc::tile_votes(W, A.thT, ns, RB, P16, wb, c0, m, kk, div, vthr, votes);
      } else {
        if constexpr (MASK) {
          if (dead) continue;
        }
        tot = Sc::tile_mean(W, A.thT, ns, RB, P16, wb, c0, m, kk, div);
      }
      if (prev_ct >= 0) finish(prev, prev_votes, prev_blk, prev_ct);
      prev = tot;
      prev_ct = ct;
      if constexpr (VOTES && ENS) prev_votes = votes;
      if constexpr (MASK) prev_blk = blk;
    }
    if (prev_ct >= 0) finish(prev, prev_votes, prev_blk, prev_ct);
  }
}

template <int KS, bool ENS, class BeginItem>
__device__ __forceinline__ void sweep(const SweepArgs& A, Head* st, double* W, unsigned* bm,
                                      BeginItem&& begin_item) {
  sweep_impl<KS, ENS, false, false>(A, st, W, bm, 0.0, nullptr, 0, nullptr, static_cast<BeginItem&&>(begin_item));
}

template <int KS, bool ENS, class BeginItem>
__device__ __forceinline__ void sweep_votes(const SweepArgs& A, Head* st, double* W, unsigned* bm, double vthr,
                                            BeginItem&& begin_item) {
  sweep_impl<KS, ENS, true, false>(A, st, W, bm, vthr, nullptr, 0, nullptr, static_cast<BeginItem&&>(begin_item));
}

// mask: [P16][MW] words, never null; mrow: MW words of the kernel's LDS.
template <int KS, bool ENS, class BeginItem>
__device__ __forceinline__ void sweep_masked(const SweepArgs& A, Head* st, double* W, unsigned* bm,
                                             const unsigned* mask, int MW, unsigned* mrow, BeginItem&& begin_item) {
  sweep_impl<KS, ENS, false, true>(A, st, W, bm, 0.0, mask, MW, mrow, static_cast<BeginItem&&>(begin_item));
}

// Both: the masked vote scan.  The votes byte and the blocked bits of a tile are kept and handed over
// together, one tile late; a dead tile is left before tile_votes, so it touches neither.
template <int KS, bool ENS, class BeginItem>
__device__ __forceinline__ void sweep_votes_masked(const SweepArgs& A, Head* st, double* W, unsigned* bm, double vthr,
                                                   const unsigned* mask, int MW, unsigned* mrow,
                                                   BeginItem&& begin_item) {
  sweep_impl<KS, ENS, true, true>(A, st, W, bm, vthr, mask, MW, mrow, static_cast<BeginItem&&>(begin_item));
}

}  // namespace scan_sweep

#endif  // MMSBM_SCAN_SWEEP_H
