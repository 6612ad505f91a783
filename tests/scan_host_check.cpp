// Host-side table of the scan families' row-block rule (csrc/scan_host.h pick_wb), built and run
// by tests/test_scan_rule_host.py on the CPU: no HIP call is made.  For both constant pairs (the
// census-like families: 1 W row per row b, scan_score::W_LDS_MAX; the partner scan: 2 and 96 KiB),
// every K in 1..32 and every ns in 1..64 it prints one line
//   <rows_per_b> <limit> <K> <ns> <WB> <w_bytes>
// with WB = 0 where pick_wb refuses the ensemble (MMSBM_ERR_UNSUPPORTED); the shape goes through
// scan_host::scan_shape, so the rounding of K is the product's.  A return code that is neither
// MMSBM_OK nor MMSBM_ERR_UNSUPPORTED, or a refusal without a message, ends it with "FAIL" (exit 1).
#include <cstdio>

#include "../trigenicinteractionpredictor_amd/csrc/scan_host.h"
#include "../trigenicinteractionpredictor_amd/csrc/scan_score.h"

static int g_K = 1, g_B = 1, g_fails = 0, g_last_code = 0;

int mmsbm_detail_fail(int code, const char* msg) {
  g_last_code = code;
  g_fails += msg && msg[0] ? 1 : 0;
  return code;
}

int mmsbm_detail_scan_shape(const mmsbm_ctx*, int* device, int* K, int* R, int* B, int* P, int* nact, int* ncu) {
  *device = 0, *K = g_K, *R = 2, *B = g_B, *P = 70, *nact = g_B, *ncu = 256;
  return MMSBM_OK;
}

int main() {
  const struct {
    int rows_per_b;
    size_t limit;
    const char* what;
  } fam[2] = {{1, (size_t)scan_score::W_LDS_MAX, "census"}, {2, (size_t)96 * 1024, "the partner scan"}};
  for (const auto& f : fam)
    for (g_K = 1; g_K <= MMSBM_MAX_K; ++g_K)
      for (int ns = 1; ns <= 64; ++ns) {
        g_B = ns;
        scan_host::ScanShape sh;
        if (scan_host::scan_shape(nullptr, f.what, &sh) != MMSBM_OK) return printf("FAIL shape %d %d\n", g_K, ns), 1;
        int WB = -1;
        size_t w_bytes = 0;
        const int before = g_fails;
        const int rc = scan_host::pick_wb(sh, f.what, f.rows_per_b, ns, f.limit, &WB, &w_bytes);
        if (rc == MMSBM_ERR_UNSUPPORTED) {
          if (g_fails != before + 1 || g_last_code != rc) return printf("FAIL message %d %d\n", g_K, ns), 1;
          WB = 0;
        } else if (rc != MMSBM_OK || g_fails != before) {
          return printf("FAIL rc %d %d %d\n", g_K, ns, rc), 1;
        }
        printf("%d %zu %d %d %d %zu\n", f.rows_per_b, f.limit, g_K, ns, WB, w_bytes);
      }
  return 0;
}
