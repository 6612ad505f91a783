// Host-side table of the top-N scans' plan (csrc/scan_topn.h make_plan, workspace_bytes), built and
// run by tests/test_scan_topn_host.py on the CPU: no HIP call is made.  For every K in {1, 10, 32},
// B in {1, 8}, P in {0, 2, 3, 16, 17, 199, 200, 1500, 2000000}, N in {1, 256, 257, 1024, 1025,
// 2048, 2049, 4096} and ncu in {32, 64, 256} it prints one line
//   plan <K> <B> <P> <N> <ncu> <cap> <G> <G2> <total> <thT> <T> <cs> <ck> <ls0> <lk0> <ln0> <ls1> <lk1> <ln1>
// and, for each of the three family names and each refused input, one line
//   refuse <N> <P> <rc> <messages> <family name>
// where <messages> counts the non-empty messages the call left in the error channel.  A plan that
// is refused, that names N or the family's shape otherwise than asked, or whose total differs from
// workspace_bytes ends the program with "FAIL" (exit 1).
#include <cstdio>

#include "../trigenicinteractionpredictor_amd/csrc/scan_topn.h"

static int g_K = 1, g_B = 1, g_P = 0, g_ncu = 256, g_fails = 0;

int mmsbm_detail_fail(int code, const char* msg) {
  g_fails += msg && msg[0] ? 1 : 0;
  return code;
}

int mmsbm_detail_scan_shape(const mmsbm_ctx*, int* device, int* K, int* R, int* B, int* P, int* nact, int* ncu) {
  *device = 0, *K = g_K, *R = 2, *B = g_B, *P = g_P, *nact = g_B, *ncu = g_ncu;
  return MMSBM_OK;
}

int main() {
  const mmsbm_ctx* ctx = reinterpret_cast<const mmsbm_ctx*>(&g_K);  // never dereferenced: the shape is stubbed
  const char* const whats[3] = {"scan", "the quorum scan", "the dispute scan"};
  const int Ks[] = {1, 10, 32}, Bs[] = {1, 8}, Ps[] = {0, 2, 3, 16, 17, 199, 200, 1500, 2000000};
  const int Ns[] = {1, 256, 257, 1024, 1025, 2048, 2049, 4096}, ncus[] = {32, 64, 256};
  for (int K : Ks)
    for (int B : Bs)
      for (int P : Ps)
        for (int N : Ns)
          for (int ncu : ncus) {
            g_K = K, g_B = B, g_P = P, g_ncu = ncu;
            scan_topn::TopNPlan p;
            int64_t bytes = -1;
            if (scan_topn::make_plan(ctx, whats[0], N, &p) != MMSBM_OK || g_fails ||
                scan_topn::workspace_bytes(ctx, whats[0], N, &bytes) != MMSBM_OK || bytes != (int64_t)p.total ||
                p.N != N || p.sh.K != K || p.sh.B != B || p.sh.P != P || p.sh.ncu != ncu)
              return printf("FAIL plan %d %d %d %d %d\n", K, B, P, N, ncu), 1;
            printf("plan %d %d %d %d %d %d %d %d %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", K, B, P, N, ncu, p.cap,
                   p.G, p.G2, p.total, p.off_thT, p.off_T, p.off_cs, p.off_ck, p.off_ls[0], p.off_lk[0], p.off_ln[0],
                   p.off_ls[1], p.off_lk[1], p.off_ln[1]);
          }
  g_K = 10, g_B = 8, g_ncu = 256;
  const int refused[3][2] = {{0, 1500}, {4097, 1500}, {16, 2000001}};  // (N, P)
  for (const char* what : whats)
    for (const auto& r : refused) {
      g_P = r[1];
      int64_t bytes = -1;
      const int before = g_fails;
      const int rc = scan_topn::workspace_bytes(ctx, what, r[0], &bytes);
      if (bytes != -1) return printf("FAIL bytes written %d %d\n", r[0], r[1]), 1;
      printf("refuse %d %d %d %d %s\n", r[0], r[1], rc, g_fails - before, what);
    }
  return 0;
}
