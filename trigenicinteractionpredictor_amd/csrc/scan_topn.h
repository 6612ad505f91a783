// scan_topn.h — the top-N machinery shared by the three scans that pick the exact top N over every
// triple (scan.hip, scan_quorum.hip, scan_spread.hip): the constants, the plan with its workspace
// layout, the LDS sizing, the fields their kernels' argument structs have in common, the merge
// kernel and the host loop over the seeding pass, the full pass and the merge levels.  A family
// keeps its kernels, its own argument checks and the lambda that launches its kernel; the partner
// and screen scans (a query dimension in their merge) have plans and merges of their own.
//
// `what` is the family's name as its messages carry it: "scan", "the quorum scan", "the dispute scan".
#ifndef MMSBM_SCAN_TOPN_H
#define MMSBM_SCAN_TOPN_H

#include "scan_host.h"
#include "scan_score.h"
#include "scan_select.h"

namespace scan_topn {

using namespace scan_host;
using namespace scan_select;

constexpr int TOPN_MAX_N = 4096;  // documented cap of N (include/mmsbm.h, mmsbm_scan_max_n)
constexpr int SEED_STRIDE = 61;   // the seeding pass scans every 61st item (prime: spreads over a and b)
constexpr int SEED_MIN_P = 200;   // below it one pass: the seeding launches would cost more than they save

struct TopNPlan {
  ScanShape sh;
  int N, cap, G, G2;
  size_t off_thT, off_T, off_cs, off_ck, off_ls[2], off_lk[2], off_ln[2], total;
};

// Everything that sizes the workspace follows the context's shape and N only (not the sample
// argument), so one workspace serves every call of that shape.
inline int make_plan(const mmsbm_ctx* c, const char* what, int N, TopNPlan* p) {
  ScanShape& sh = p->sh;
  if (int rc = scan_shape(c, what, &sh)) return rc;
  if (N < 1) return fail(MMSBM_ERR_INVALID, "N=%d < 1", N);
  if (N > TOPN_MAX_N) return fail(MMSBM_ERR_UNSUPPORTED, "N=%d above the scan's cap of %d", N, TOPN_MAX_N);
  if (int rc = packed_keys_fit(sh)) return rc;
  p->N = N;
  p->cap = 512;  // the candidate buffer: a power of two >= 2 N
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

// The body of a family's *_workspace_bytes entry point.
inline int workspace_bytes(const mmsbm_ctx* c, const char* what, int N, int64_t* bytes) {
  if (!c || !bytes) return fail(MMSBM_ERR_INVALID, "null argument");
  TopNPlan p;
  if (int rc = make_plan(c, what, N, &p)) return rc;
  *bytes = (int64_t)p.total;
  return MMSBM_OK;
}

// Dynamic LDS of a scan kernel (Sel, the W rows, `extra` bytes in front of the candidate buffer: a
// masked kernel's mask row, which may move the buffer to the workspace, which holds it anyway) and
// of the merge kernel (Sel and the buffer).
struct TopNLds {
  bool cand_lds;  // the candidate buffer fits the LDS behind W
  int lds, merge_lds;
};

inline TopNLds lds_sizes(const TopNPlan& p, size_t w_bytes, size_t extra) {
  const size_t cand_bytes = (size_t)p.cap * 16;
  TopNLds l;
  l.cand_lds = sizeof(Sel) + w_bytes + extra + cand_bytes <= (size_t)LDS_MAX;
  l.lds = (int)(sizeof(Sel) + w_bytes + extra + (l.cand_lds ? cand_bytes : 0));
  l.merge_lds = (int)(sizeof(Sel) + cand_bytes);
  return l;
}

// The fields that ScanArgs, QuorumArgs and SpreadArgs have in common, by name: each struct keeps
// its own members and order.  The pass loop hands `stride` to the family's launch.
template <class Args>
void fill_common(Args& a, const TopNPlan& p, const TopNLds& l, void* ws, const int64_t* known, int64_t n_known,
                 int ns, int WB, int stride) {
  char* w = (char*)ws;
  a.thT = (const double*)(w + p.off_thT);
  a.T = (const double*)(w + p.off_T);
  a.known = (const long long*)known;
  a.n_known = n_known;
  a.cand_s = l.cand_lds ? nullptr : (double*)(w + p.off_cs);
  a.cand_k = l.cand_lds ? nullptr : (long long*)(w + p.off_ck);
  a.list_s = (double*)(w + p.off_ls[0]);
  a.list_k = (long long*)(w + p.off_lk[0]);
  a.list_n = (int*)(w + p.off_ln[0]);
  a.shared = (unsigned long long*)w;
  a.K = p.sh.K, a.P = p.sh.P, a.P16 = p.sh.P16, a.ns = ns, a.N = p.N, a.cap = p.cap, a.WB = WB;
  a.stride = stride;
}

namespace {

// ------------------------------------------------------------------------------------------
// Merge: workgroup w keeps the best N of lists [FAN w, FAN (w + 1)); the last level (one
// workgroup) writes the result: scores, gene ids in key order, count, NaN / -1 tail.
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

__global__ __launch_bounds__(NT) void merge_kernel(MergeArgs A) {
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

}  // namespace

// One top-N call on stream `s`, after the family's checks: zero the published bound, prep
// (P >= 3), then the passes.  Pass 0 (`seed` and P >= SEED_MIN_P only) seeds the bound: the same
// scan and merge over every SEED_STRIDE-th item, whose exact N-th score (a subset's N-th best is a
// lower bound of the whole's) is published instead of written out.  Pass 1 scans every item and
// starts from that bound, so it appends about N SEED_STRIDE candidates in all instead of filling
// every workgroup's buffer from nothing.  The bound only prunes: the result does not depend on it.
// launch(n_lists, stride) launches the family's kernel on n_lists workgroups (at most G <= p.G,
// for which the lists and buffers are sized) and returns its code.
template <class Launch>
int run_passes(const TopNPlan& p, int merge_lds, bool seed, int G, const int32_t* order, const double* theta,
               const double* pr, int ns, int s0, void* ws, double* out_scores, int32_t* out_ids,
               int64_t* out_count, hipStream_t s, Launch&& launch) {
  const ScanShape& sh = p.sh;
  DeviceGuard g(sh.device);
  char* w = (char*)ws;
  HIP_TRY(hipMemsetAsync(w, 0, 256, s));
  int* ln[2] = {(int*)(w + p.off_ln[0]), (int*)(w + p.off_ln[1])};
  double* ls[2] = {(double*)(w + p.off_ls[0]), (double*)(w + p.off_ls[1])};
  long long* lk[2] = {(long long*)(w + p.off_lk[0]), (long long*)(w + p.off_lk[1])};
  if (sh.P >= 3) {
    scan_score::scan_prep_kernel<<<dim3(sh.P16, ns), NT, 0, s>>>(order, theta, pr, (double*)(w + p.off_thT),
                                                                 (double*)(w + p.off_T), sh.K, sh.KP, sh.R, sh.P,
                                                                 sh.P16, s0);
    HIP_TRY(hipGetLastError());
  }
  for (int pass = (seed && sh.P >= SEED_MIN_P) ? 0 : 1; pass < 2; ++pass) {
    const bool seeding = pass == 0;
    int n_lists = 0;
    if (sh.P >= 3) {
      n_lists = seeding ? std::min(G, sh.ncu) : G;
      if (int rc = launch(n_lists, seeding ? SEED_STRIDE : 1)) return rc;
    }
    int cur = 0;
    for (;;) {
      const bool last = n_lists <= FAN;
      MergeArgs ma{};
      ma.in_s = ls[cur], ma.in_k = lk[cur], ma.in_n = ln[cur], ma.n_in = n_lists;
      if (!last) ma.out_s = ls[cur ^ 1], ma.out_k = lk[cur ^ 1], ma.out_n = ln[cur ^ 1];
      ma.order = order, ma.scores = out_scores, ma.ids = out_ids, ma.count = (long long*)out_count;
      ma.shared = (seeding && last) ? (unsigned long long*)w : nullptr;
      ma.N = p.N, ma.cap = p.cap, ma.P = std::max(sh.P, 1);
      const int n_out = last ? 1 : (n_lists + FAN - 1) / FAN;
      if (int rc = launch_lds(merge_kernel, n_out, merge_lds, s, ma)) return rc;
      if (last) break;
      n_lists = n_out;
      cur ^= 1;
    }
  }
  return MMSBM_OK;
}

}  // namespace scan_topn

#endif  // MMSBM_SCAN_TOPN_H
