// scan_host.h — the host prologue shared by the four scan families (scan.hip, partners.hip,
// census.hip, pair_census.hip): the error channel, the device guard, the context's shape with its
// checks and roundings, the thT / T workspace pair, the per-call argument checks, the row-block
// width, the launch with large dynamic LDS, the dispatch on K, the measurement variables and the
// grid of the two censuses' sweep.
//
// `what` is the family's name as its messages carry it: "scan", "the partner scan", "census",
// "pair census".  Every check returns the code the family has always returned for that input; the
// families run their own checks (N, M, Q, null pointers) between these in the order they always had.
#ifndef MMSBM_SCAN_HOST_H
#define MMSBM_SCAN_HOST_H

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <type_traits>

#include "mmsbm.h"
#include "scan_select.h"

int mmsbm_detail_fail(int code, const char* msg);  // mmsbm.hip: the library's error channel
int mmsbm_detail_scan_shape(const mmsbm_ctx* c, int* device, int* K, int* R, int* B, int* P, int* nact,
                            int* ncu);

namespace scan_host {

using scan_select::NT;

inline int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  return mmsbm_detail_fail(code, buf);
}

#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess) return scan_host::fail(MMSBM_ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DeviceGuard() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// The context's shape as every family plans with it: KP = K rounded up to 4, P16 = P rounded up to
// 16 (at least 16), nact = the active prefix of the B samples, ncu = the device's compute units.
struct ScanShape {
  int device, K, KP, R, B, P, P16, nact, ncu;
};

inline int scan_shape(const mmsbm_ctx* c, const char* what, ScanShape* sh) {
  mmsbm_detail_scan_shape(c, &sh->device, &sh->K, &sh->R, &sh->B, &sh->P, &sh->nact, &sh->ncu);
  if (sh->K < 1 || sh->K > MMSBM_MAX_K)
    return fail(MMSBM_ERR_UNSUPPORTED, "K=%d outside [1, %d]: call mmsbm_set_shape", sh->K, MMSBM_MAX_K);
  if (sh->R < 2 || sh->B < 1 || sh->P < 0)
    return fail(MMSBM_ERR_INVALID, "%s needs R >= 2, B >= 1 (mmsbm_set_shape)", what);
  sh->KP = (sh->K + 3) / 4 * 4;
  sh->P16 = std::max(16, (sh->P + 15) / 16 * 16);
  return MMSBM_OK;
}

// A triple's packed key (a P + b) P + c must fit 63 bits (the pair census has its own, lower cap).
inline int packed_keys_fit(const ScanShape& sh) {
  if ((long long)sh.P > 2000000) return fail(MMSBM_ERR_UNSUPPORTED, "P=%d: packed keys overflow", sh.P);
  return MMSBM_OK;
}

// The pair mask of the masked families (include/mmsbm.h): uint32[P16][MW], MW = ceil(P16 / 32) words
// per row, for P up to the pair census's cap (a row is at most 2 KiB of LDS, the mask 32 MiB).
constexpr int PAIR_MASK_MAX_P = 16384;
inline int pair_mask_words(const ScanShape& sh, const char* what, int* MW) {
  if (sh.P > PAIR_MASK_MAX_P)
    return fail(MMSBM_ERR_UNSUPPORTED, "%s: P=%d above the pair mask's cap of %d", what, sh.P, PAIR_MASK_MAX_P);
  *MW = (sh.P16 + 31) / 32;
  return MMSBM_OK;
}

// A masked call's mask: the cap on P, then the pointer (the unmasked call exists for "no mask").
inline int check_pair_mask(const ScanShape& sh, const char* what, const uint32_t* mask, int* MW) {
  if (int rc = pair_mask_words(sh, what, MW)) return rc;
  if (!mask) return fail(MMSBM_ERR_INVALID, "%s: null pair mask (the unmasked call takes none)", what);
  if ((uintptr_t)mask & 3) return fail(MMSBM_ERR_INVALID, "%s: misaligned pair mask", what);
  return MMSBM_OK;
}

// thT[B][KP][P16] and T[B][P][K][KP] (scan_score.h) from `off` on, each 256-byte aligned.
inline void score_workspace(const ScanShape& sh, size_t& off, size_t* off_thT, size_t* off_T) {
  const size_t B = sh.B, P = sh.P, K = sh.K, KP = sh.KP, P16 = sh.P16;
  *off_thT = off, off = align256(off + sizeof(double) * B * KP * P16);
  *off_T = off, off = align256(off + sizeof(double) * B * P * K * KP);
}

// The checks of one call: the known-key table (null with 0 keys where the family has its own), the
// sample (-1: the ensemble of the active prefix) and the workspace of `total` bytes, which
// `remedy` sizes.  Yields the number of samples scored and the first one's slot.
inline int check_call(const ScanShape& sh, const char* what, const char* remedy, const int64_t* known,
                      int64_t n_known, int sample, const void* ws, int64_t ws_bytes, size_t total, int* ns,
                      int* s0) {
  if (n_known < 0 || (n_known > 0 && !known)) return fail(MMSBM_ERR_INVALID, "bad known-key table");
  if (sample < -1 || sample >= sh.nact)
    return fail(MMSBM_ERR_INVALID, "sample %d outside the active prefix [0, %d)", sample, sh.nact);
  if (!ws || ws_bytes < (int64_t)total || ((uintptr_t)ws & 15))
    return fail(MMSBM_ERR_INVALID, "%s: workspace missing, misaligned or too small (%s)", what, remedy);
  *ns = sample >= 0 ? 1 : sh.nact;
  *s0 = sample >= 0 ? sample : 0;
  return MMSBM_OK;
}

// The widest row block (WB b-tiles of 16 rows, a power of two <= 4) whose W rows (rows_per_b per
// row b, KP + 2 doubles each, `ns` samples) fit `limit` bytes of LDS; an ensemble that does not fit
// at WB = 1 is unsupported.
inline int pick_wb(const ScanShape& sh, const char* what, int rows_per_b, int ns, size_t limit, int* WB,
                   size_t* w_bytes) {
  const size_t row_block = sizeof(double) * rows_per_b * ns * 16 * (sh.KP + 2);
  *WB = 4;
  while (*WB > 1 && row_block * *WB > limit) *WB >>= 1;
  *w_bytes = row_block * *WB;
  if (*w_bytes > limit)
    return fail(MMSBM_ERR_UNSUPPORTED,
                "%s: an ensemble of %d samples at K=%d exceeds the LDS tile: take the samples one by one", what, ns,
                sh.K);
  return MMSBM_OK;
}

// Launch `kernel` with NT threads and `lds` bytes of dynamic LDS (above 64 KiB it has to be allowed).
template <class Args>
int launch_lds(void (*kernel)(Args), dim3 grid, int lds, hipStream_t s, const Args& a) {
  if (lds > 64 * 1024)
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                lds));
  kernel<<<grid, NT, lds, s>>>(a);
  HIP_TRY(hipGetLastError());
  return MMSBM_OK;
}

// f(std::integral_constant<int, KS>{}) for KS = ks in [1, 8] (KP / 4: MMSBM_MAX_K = 32).
template <class F>
int dispatch_ks(int ks, F&& f) {
  switch (ks) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 5: return f(std::integral_constant<int, 5>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 7: return f(std::integral_constant<int, 7>{});
    default: return f(std::integral_constant<int, 8>{});
  }
}

// A measurement variable's integer value (`unset` when it is not in the environment).
inline long long env_override(const char* name, long long unset) {
  const char* e = getenv(name);
  return e ? atoll(e) : unset;
}

// The number of workgroups of a triangle sweep (scan_sweep.h): 4 per compute unit, no more than
// there are items (a, a block of 16 WB rows b); `env` names the measurement variable that
// overrides it.
constexpr int GRID_MAX = 1 << 20;
inline int sweep_grid(const ScanShape& sh, int WB, const char* env) {
  const long long items = std::max<long long>(1, (long long)sh.P * ((sh.P + 16 * WB - 1) / (16 * WB)));
  const long long g = env_override(env, 0);
  return (int)(g >= 1 ? std::min<long long>(g, GRID_MAX) : std::min<long long>(4LL * sh.ncu, items));
}

}  // namespace scan_host

#endif  // MMSBM_SCAN_HOST_H
