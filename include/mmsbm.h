/*
 * mmsbm.h — C ABI of the MI355X MMSBM EM engine (libmmsbm.so).
 *
 * Drop-in boundary for the triplet-link E/M loop of
 * AleixMT/TrigenicInteractionPredictor, src/TrigenicInteractionPredictor.py.
 * The reference boundary is a Python method API, not an FFI; each entry point
 * below names the reference method it replaces.  The Python host mirror
 * (trigenicinteractionpredictor_amd/model.py, class Model) binds these through
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *  - every call returns MMSBM_OK (0) or a negative MMSBM_ERR_* code;
 *    mmsbm_last_error() returns the message of the last failure (thread-local);
 *  - pointers whose name ends in _host are HOST arrays; every other array
 *    pointer is a DEVICE pointer (memory owned by the caller, e.g. PyTorch
 *    tensors);
 *  - kernels are enqueued on the caller's hipStream_t (passed as void*); the
 *    setup calls (set_links, set_degree, set_workspace) synchronise;
 *  - every call runs on the context's device and restores the caller's current
 *    device on return;
 *  - a context is not thread-safe: one host thread per context.
 *
 * Device layouts
 *  - theta  f64[B][P][K]          membership vectors of B batched samples (:117-121)
 *  - pr     f64[B][R][K][K][K]    rating-major copy of the reference's
 *           pr[K][K][K][R] (:124-139)
 *  The engine's own work plan (observation streams ordered by each slot's gene,
 *  DESIGN.md) is built inside mmsbm_set_links from the host link table.
 */
#ifndef MMSBM_H
#define MMSBM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MMSBM_OK 0
#define MMSBM_ERR_INVALID -1      /* bad argument / call order */
#define MMSBM_ERR_HIP -2          /* a HIP runtime call failed */
#define MMSBM_ERR_ZERO_DEGREE -3  /* a gene has no train link: the reference raises
                                     ZeroDivisionError at :1018 */
#define MMSBM_ERR_UNSUPPORTED -4  /* shape outside the compiled kernel set */

#define MMSBM_CHUNK 4             /* observations per MFMA k-step (one pivot gene each) */
#define MMSBM_MAX_K 32
#define MMSBM_SET_TRAIN 0         /* `links` (:57) */
#define MMSBM_SET_TEST 1          /* `test_links` (:61) */

typedef struct mmsbm_ctx mmsbm_ctx;

int mmsbm_version(void);
int mmsbm_chunk(void);
/* 16 hex digits naming the build (sha256 of the sources, headers, arch and flags): profile
 * records are stamped with it so a measurement can be matched to the library it came from. */
const char *mmsbm_build_id(void);
const char *mmsbm_last_error(void);

/* Context = one GPU + one problem shape.  Replaces the per-process `Model()`
 * state of :39-88 for the hot path. */
int mmsbm_create(int device, mmsbm_ctx **out);
int mmsbm_destroy(mmsbm_ctx *ctx);

/* K groups, R ratings (2 in the reference, :79), B batched samples
 * (independent restarts, :1253), P genes (:413), eps (:88).  Changing K, R or P
 * drops the link sets, the degree and the workspace (call mmsbm_set_links and
 * mmsbm_set_workspace again); changing B drops the workspace.
 * Accepted: 1 <= K <= MMSBM_MAX_K and 2 <= R <= 8 (MMSBM_ERR_UNSUPPORTED outside either
 * range; the context keeps its previous shape), eps >= 0.  A rating no train link
 * observes (counts_host[e][r] == 0 for every e) is valid: its slice pr[b][r] becomes
 * exactly 0 at the first iteration and stays 0.  Every kernel takes eps from here; none
 * assumes the reference's 1e-10. */
int mmsbm_set_shape(mmsbm_ctx *ctx, int32_t K, int32_t R, int32_t B, int32_t P, double eps);

/* One link set (MMSBM_SET_TRAIN = `links`, MMSBM_SET_TEST = `test_links`) as the
 * reference holds it after get_traintest (:321-423), in dict insertion order:
 * ids_host[E][3] = the key's gene ids in its string-sorted order ('10_2_9' ->
 * 10, 2, 9; :349-358), counts_host[E][R] = links[key] (:360-368).  Builds the
 * device work plan.  For the train set it also computes the degree (the
 * reference's `counter`, :986-994: one per link slot) unless mmsbm_set_degree
 * fixed it.  Invalidates the workspace (query mmsbm_workspace_bytes again). */
int mmsbm_set_links(mmsbm_ctx *ctx, int32_t which, const int32_t *ids_host,
                    const int32_t *counts_host, int64_t E);

/* Kernel family of the small-K plans (K <= 12; one family above): the three-stream fused
 * E-step (SK_U) or the stream-0 E-step with Y entries (SK_Y).  Both follow the reference's sums
 * (:996-1028) and agree with it to ~1e-12; their sums are ordered differently, so a sample's bits
 * depend on the family, and within one family on nothing else (not B, not the sample's slot, not
 * the rank).  AUTO picks from B at every mmsbm_set_shape (B = 1: SK_U, the one-sample latency
 * winner; B >= 2: SK_Y, the throughput winner); a driver whose engines hold different B for one
 * run (a ragged last batch, ranks with unequal shares, a pool that shrinks) fixes the family from
 * its configured batch instead, so every sample of the run gets the same bits.  A change of the
 * effective family drops the link plans (call mmsbm_set_links again).  The environment variable
 * MMSBM_SK_Y=0/1 overrides it (measurement).  Replaces nothing in the reference (a scheduling
 * choice of this engine). */
#define MMSBM_FAMILY_AUTO 0
#define MMSBM_FAMILY_SKU 1
#define MMSBM_FAMILY_SKY 2
int mmsbm_set_family(mmsbm_ctx *ctx, int32_t family);

/* Active samples: mmsbm_iterate, mmsbm_loglik, mmsbm_accumulate, mmsbm_mstep and mmsbm_predict
 * process samples [0, n) of the B and leave the others untouched (n = 0 or n >= B: all B; the
 * default).  A restart driver that retires converged samples compacts the live ones to the front
 * and shrinks n instead of iterating finished slots (the reference ends a sample at convergence,
 * :1270-1276).  mmsbm_set_shape resets it to B. */
int mmsbm_set_active(mmsbm_ctx *ctx, int32_t n);

/* deg_host[P]: the degree the M-step divides by (:1016-1018) — for a
 * link-sharded rank the counter over ALL train links, not its own block.  A
 * zero makes mmsbm_iterate / mmsbm_mstep fail with MMSBM_ERR_ZERO_DEGREE.
 * The degree is pinned for the NEXT mmsbm_set_links(MMSBM_SET_TRAIN) only: a
 * train link set given without a preceding mmsbm_set_degree is counted afresh. */
int mmsbm_set_degree(mmsbm_ctx *ctx, const int32_t *deg_host);

/* Scratch the engine needs (c per observation, partial rows, S partials). */
int mmsbm_workspace_bytes(const mmsbm_ctx *ctx, int64_t *bytes);
int mmsbm_set_workspace(mmsbm_ctx *ctx, void *ws, int64_t bytes);

/* n_iters EM iterations on all B samples, in place.
 * Replaces Model.make_iteration (:984-1043) called n_iters times. */
int mmsbm_iterate(mmsbm_ctx *ctx, double *theta, double *pr, int32_t n_iters, void *stream);

/* Log-likelihood of link set `which` for every sample into out[B] (device).
 * Replaces Model.compute_likelihood(selected_set) (:952-974). */
int mmsbm_loglik(mmsbm_ctx *ctx, int32_t which, const double *theta, const double *pr,
                 double *out, void *stream);

/* P(r = 1) for n rows of ids int32[n][3] into out[B][n] (device); an id outside
 * [0, P) gives NaN.  Replaces Model.do_prediction (:530-547), used by
 * calculate_test_set_results (:557-569). */
int mmsbm_predict(mmsbm_ctx *ctx, const int32_t *ids, int64_t n, const double *theta,
                  const double *pr, double *out, void *stream);

/* Genome-wide scan: the exact top N of Model.do_prediction (:530-547, no eps) over every triple of
 * DISTINCT genes, each taken once in the reference's key order (:349-358: ids sorted as decimal
 * strings).  order[P] (device) = the gene ids sorted by str(id); a triple is three positions
 * a < b < c of it, its score do_prediction(order[a], order[b], order[c]) and its packed key
 * (a P + b) P + c.  known (device; NULL = none) = n_known packed keys, sorted ascending, of triples
 * to skip (the measured ones); keys of no triple are ignored.  sample >= 0 scans that slot of the
 * active prefix (mmsbm_set_active); -1 scans the ensemble: the scores of slots [0, n_active) added
 * in slot order, then divided by n_active (the per-triplet mean of testResultsReducer.py:153-184).
 * Result (device): the first *out_count rows of out_scores f64[N] and out_ids int32[N][3] (gene
 * ids in key order) hold the best triples under the total order (score descending; equal scores:
 * smaller packed key first); *out_count < N when fewer are eligible (P < 3: 0); the tail is
 * NaN / -1.  That list is unique, so it does not depend on the grid, the device or the batch the
 * sample sits in.  1 <= N <= mmsbm_scan_max_n() (4096); above it MMSBM_ERR_UNSUPPORTED, as for an
 * ensemble whose W tile of 16 rows exceeds 64 KiB of LDS: n_active (4 ceil(K / 4) + 2) > 512 (scan
 * the slots one by one).
 * ws: mmsbm_scan_workspace_bytes(ctx, N) bytes of device scratch, 16-byte aligned, the caller's
 * (independent of mmsbm_set_workspace).  theta and pr are only read; all launches go to `stream`
 * and nothing synchronises.  Needs R >= 2.  The caller guarantees that order is a permutation of
 * [0, P) (ids outside it score as zero rows).  Replaces nothing in the reference, which predicts
 * listed triplets only (calculate_test_set_results, :557-569). */
int mmsbm_scan_max_n(void);
int mmsbm_scan_workspace_bytes(const mmsbm_ctx *ctx, int32_t N, int64_t *bytes);
int mmsbm_scan_topn(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                    const double *theta, const double *pr, int32_t sample, int32_t N, void *ws,
                    int64_t ws_bytes, double *out_scores, int32_t *out_ids, int64_t *out_count,
                    void *stream);

/* Pair-masked genome-wide scan: mmsbm_scan_topn with the pair mask of mmsbm_scan_census_masked behind
 * n_known, under that call's layout and rule: mask (device) = uint32[rows][words_per_row] of
 * mmsbm_pair_mask_shape in rank positions, bit y of row x set = the pair (x, y) is blocked, only
 * x < y read.  A triple a < b < c is eligible when it is eligible for the unmasked call and none of
 * (a, b), (a, c), (b, c) is blocked.  Everything else is the unmasked call's: the arguments, the
 * result rows, the total order, the cap on N, the measurement variables (MMSBM_SCAN_SELECT=0: the
 * bare score phase; MMSBM_SCAN_GRID=<workgroups> lowers the grid, on which neither call's list
 * depends) and the workspace (mmsbm_scan_workspace_bytes, unchanged).  A listed score carries the bits mmsbm_scan_topn gives that
 * triple, so an all-zero mask returns the unmasked list, and a mask returns the unmasked call's list
 * with the keys of every triple that contains a blocked pair added to `known`: the exact, unique
 * top N of the masked-eligible triples (the pruning bounds, the seeding pass's included, are formed
 * from masked-eligible candidates only), *out_count < N when fewer are eligible.  P <= 16384
 * (MMSBM_ERR_UNSUPPORTED above); a NULL mask is MMSBM_ERR_INVALID: the unmasked call exists for that.
 * Every check comes before any device call.  Replaces nothing in the reference. */
int mmsbm_scan_topn_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                           int64_t n_known, const uint32_t *mask, const double *theta,
                           const double *pr, int32_t sample, int32_t N, void *ws, int64_t ws_bytes,
                           double *out_scores, int32_t *out_ids, int64_t *out_count, void *stream);

/* Partner scan: for each query gene, the exact top N of Model.do_prediction (:530-547, no eps) over
 * the pairs of other genes it forms a triple with.  Notation as for mmsbm_scan_topn: order[P]
 * (device) = the gene ids sorted by str(id), Th' = theta in that order, p_1 the rating-1 lattice, a
 * triple three rank positions sorted ascending with the packed key (a P + b) P + c and the score
 * do_prediction(order[a], order[b], order[c]).
 * Candidates of a query at rank position q: every pair of positions b < c with b != q and c != q;
 * the triple is {q, b, c} sorted.  Its score factors through the query's slot of p_1:
 *   q < b < c:  S = Th'[b] T1_q Th'[c]^T,  T1_q[y][z] = sum_x Th'[q][x] p_1[x][y][z]
 *   b < q < c:  S = Th'[b] T2_q Th'[c]^T,  T2_q[x][z] = sum_y Th'[q][y] p_1[x][y][z]
 *   b < c < q:  S = Th'[b] T3_q Th'[c]^T,  T3_q[x][y] = sum_z Th'[q][z] p_1[x][y][z]
 * (two triangles and a rectangle of one P x P matrix, (P - 1)(P - 2) / 2 scores, each region a GEMM
 * of inner size K).
 * queries_host int32[Q] (HOST) = gene ids in [0, P); they may repeat and every row is answered on
 * its own.  An id outside [0, P) returns MMSBM_ERR_INVALID before anything is launched; Q = 0
 * returns MMSBM_OK and writes nothing.  The ids are copied to the workspace on `stream`.
 * Exclusion, per query in CSR form: known_off int64[Q + 1] (device) offsets into known_pairs
 * (device), query i's slice holding the sorted, unique pair keys b P + c (rank positions of the
 * other two genes, b < c) to skip.  Keys that name q or no pair are ignored.  known_off = NULL: none.
 * sample >= 0 scans that slot of the active prefix; -1 the ensemble, formed as the scan forms it:
 * each slot's tile accumulated from zero, the tiles added in slot order, divided by n_active.
 * Result (device), row i for query i: the first out_count[i] rows of out_scores f64[Q][N] and
 * out_ids int32[Q][N][3] hold the query's best candidates under the scan's total order (score
 * descending; equal scores: the smaller packed key of the TRIPLE first); out_ids are the whole
 * triple's gene ids in key order, the query included, so a row can go straight into mmsbm_predict.
 * out_count int64[Q]; the tail of a row is NaN / -1; P < 3: count 0.
 * Every sum has a fixed order and no score is formed by an atomic, and the exact top N under a total
 * order is unique: a query's list and its score bits do not depend on Q, on the other queries of
 * the call, on the grid or on the batch the sample sits in.  The scores need not equal
 * mmsbm_scan_topn's bit for bit (the contraction runs through another slot); they agree to 1e-9
 * relative.
 * 1 <= N <= mmsbm_partners_max_n() (1024: a workgroup's candidate buffer stays in the LDS); above
 * it MMSBM_ERR_UNSUPPORTED, as for an ensemble whose two W tiles of 16 rows exceed 96 KiB of LDS:
 * n_active (4 ceil(K / 4) + 2) > 384 (scan the slots one by one).  Q <= 65535.  Needs R >= 2.
 * ws: mmsbm_partners_workspace_bytes(ctx, Q, N) bytes of device scratch, 16-byte aligned, the
 * caller's; its size follows the context's shape, Q and N only.  theta and pr are only read; all
 * launches go to `stream` and nothing synchronises.  The caller guarantees that order is a
 * permutation of [0, P).  Replaces nothing in the reference. */
int mmsbm_partners_max_n(void);
int mmsbm_partners_workspace_bytes(const mmsbm_ctx *ctx, int64_t Q, int32_t N, int64_t *bytes);
int mmsbm_partners_topn(mmsbm_ctx *ctx, const int32_t *order, const int32_t *queries_host, int64_t Q,
                        const int64_t *known_off, const int64_t *known_pairs, const double *theta,
                        const double *pr, int32_t sample, int32_t N, void *ws, int64_t ws_bytes,
                        double *out_scores, int32_t *out_ids, int64_t *out_count, void *stream);

/* Pair-masked partner scan: mmsbm_partners_topn with the pair mask of mmsbm_scan_census_masked behind
 * known_pairs (the same layout; only x < y read).  A candidate pair b < c of the query at rank
 * position q is eligible when it is eligible for the unmasked call and none of {q, b}, {q, c}, (b, c)
 * is blocked; the pairs with q are read at (min, max).  Everything else is the unmasked call's: the
 * arguments, the rows, the total order, the caps, the measurement variable and the workspace
 * (mmsbm_partners_workspace_bytes, unchanged).  A listed score carries the bits mmsbm_partners_topn
 * gives that candidate, so an all-zero mask returns the unmasked rows, and a mask returns the
 * unmasked call's rows with the pair keys b P + c of every blocked candidate added to the query's
 * slice of known_pairs.  A query whose every candidate is blocked has count 0 and a NaN / -1 row; a
 * query's row still does not depend on Q, on the other queries, on the grid or on the batch.
 * P <= 16384 (MMSBM_ERR_UNSUPPORTED above); a NULL mask is MMSBM_ERR_INVALID: the unmasked call
 * exists for that.  Every check comes before any device call.  Replaces nothing in the reference. */
int mmsbm_partners_topn_masked(mmsbm_ctx *ctx, const int32_t *order, const int32_t *queries_host,
                               int64_t Q, const int64_t *known_off, const int64_t *known_pairs,
                               const uint32_t *mask, const double *theta, const double *pr,
                               int32_t sample, int32_t N, void *ws, int64_t ws_bytes,
                               double *out_scores, int32_t *out_ids, int64_t *out_count, void *stream);

/* Score census: for M thresholds, the exact number of the scan's eligible triples whose score is at
 * or above each, and the number of eligible triples.  order, known, n_known, theta, pr, sample
 * (-1: the mean over the active prefix), ws and stream mean what they mean for mmsbm_scan_topn, and
 * a triple is eligible exactly as there: rank positions a < b < c < P whose packed key is not among
 * `known`.  A score carries the same bits as in mmsbm_scan_topn (one score phase serves both), so
 * a census at the scores of a scan list returns each entry's position in that list.
 * thresholds f64[M] (device): finite and non-decreasing (the caller guarantees both; duplicates are
 * fine), 0 <= M <= mmsbm_census_max_m() (1024); above it MMSBM_ERR_UNSUPPORTED, as for K outside
 * [1, MMSBM_MAX_K] and for an ensemble whose W tile exceeds the LDS (as for the scan).  Null
 * pointers, a bad sample or a small workspace: MMSBM_ERR_INVALID.
 * Result (device) out_counts int64[M + 1]: out_counts[m], m < M = the eligible triples with
 * score >= thresholds[m]; out_counts[M] = the eligible triples in all (counted by the kernel; P < 3:
 * every count is 0).  The counts are integers combined by integer adds only (LDS and 64-bit global
 * atomics, then suffix sums); no floating-point value is summed across lanes or workgroups, so they
 * do not depend on the grid, the batch the sample sits in or the arrival order.  A count is at most
 * C(P, 3) < 2^63.
 * ws: mmsbm_census_workspace_bytes(ctx, M) bytes of device scratch, 16-byte aligned, the caller's;
 * its size follows the context's shape and M only (a workspace for M serves every smaller M).
 * theta, pr and thresholds are only read; all launches go to `stream` and nothing synchronises.
 * The environment variable MMSBM_CENSUS_GRID=<workgroups> overrides the grid (measurement; the
 * counts do not depend on it).  Needs R >= 2.  Replaces nothing in the reference. */
int mmsbm_census_max_m(void);
int mmsbm_census_workspace_bytes(const mmsbm_ctx *ctx, int32_t M, int64_t *bytes);
int mmsbm_scan_census(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                      const double *theta, const double *pr, int32_t sample,
                      const double *thresholds, int32_t M, void *ws, int64_t ws_bytes,
                      int64_t *out_counts, void *stream);

/* Pair census: the census's counts binned by pair.  For M thresholds and every pair of rank
 * positions x < y, the exact number of the scan's eligible triples that contain both x and y and
 * whose score is at or above each threshold: the number of predicted, unmeasured interactions a
 * double-mutant query (x, y) would have.  order, known, n_known, theta, pr, sample (-1: the mean over
 * the active prefix), thresholds, ws and stream mean what they mean for mmsbm_scan_census; a triple
 * is eligible exactly as there, and its score carries the same bits (one score phase serves the
 * scan, the census and this call), so for every m the sum of the result over x < y is exactly three
 * times mmsbm_scan_census's count at thresholds[m].
 * thresholds f64[M] (device): finite and non-decreasing (the caller guarantees both; duplicates are
 * fine), 0 <= M <= mmsbm_pair_census_max_m() (8: a tile with hits walks the thresholds one
 * by one); above it MMSBM_ERR_UNSUPPORTED, as for K outside [1, MMSBM_MAX_K], for an ensemble
 * whose W tile exceeds the LDS (as for the census) and for P > 16384 (a pair index x P + y stays
 * below 2^28 and the result below 8 GiB).  Null pointers, a bad sample or a small workspace:
 * MMSBM_ERR_INVALID.  Every argument is checked before any device call.
 * Result (device) out_counts int32[P][P][M], zeroed by the call: out_counts[x][y][m], x < y = the
 * eligible triples that contain the genes at rank positions x and y with score >= thresholds[m];
 * entries with x >= y stay 0.  A count is at most P - 2.  M = 0 writes nothing; P < 3: all 0.  The
 * call does not count a pair's eligible triples (P - 2 minus the known keys that contain the pair:
 * host arithmetic on `known`).
 * The counts are integers combined by integer adds only (registers, integer cross-lane moves and
 * 32-bit global atomics); no floating-point value crosses a lane, so they do not depend on the grid,
 * the batch the sample sits in or the arrival order.
 * ws: mmsbm_pair_census_workspace_bytes(ctx, M) bytes of device scratch, 16-byte aligned, the
 * caller's; its size follows the context's shape only.  theta, pr and thresholds are only read; all
 * launches go to `stream` and nothing synchronises.  The environment variable
 * MMSBM_PAIR_CENSUS_GRID=<workgroups> overrides the grid (measurement; the counts do not depend on
 * it).  Needs R >= 2.  Replaces nothing in the reference. */
int mmsbm_pair_census_max_m(void);
int mmsbm_pair_census_workspace_bytes(const mmsbm_ctx *ctx, int32_t M, int64_t *bytes);
int mmsbm_pair_census(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                      const double *theta, const double *pr, int32_t sample,
                      const double *thresholds, int32_t M, void *ws, int64_t ws_bytes,
                      int32_t *out_counts, void *stream);

/* Threshold scan: every one of the scan's eligible triples whose score is at or above one threshold,
 * listed.  The census says how many there are; this call says which.  order, known, n_known, theta,
 * pr, sample (-1: the mean over the active prefix), ws and stream mean what they mean for
 * mmsbm_scan_census; a triple is eligible exactly as there (rank positions a < b < c < P whose
 * packed key is not among `known`), and its score carries the same bits (one score phase serves the
 * scan, the censuses and this call).  A hit is an eligible triple with score >= threshold, so the
 * number of hits is exactly mmsbm_scan_census's count at that threshold.
 * Result (device): *out_count int64[1] = the number of hits, always the full number, also when it
 * exceeds `capacity`.  The first min(*out_count, capacity) rows of out_scores f64[capacity] and
 * out_keys int64[capacity] hold hits: the score and the packed key (a P + b) P + c (gene ids:
 * order[a], order[b], order[c]).  The rows come in ARRIVAL order, which follows the grid and the run
 * and may differ between two calls: only the SET of rows is defined.  When *out_count <= capacity it
 * is the complete set of hits, each exactly once; sorted under the scan's total order (score
 * descending; equal scores: smaller packed key first) it is a unique list that does not depend on
 * the grid, the device or the batch the sample sits in, and its first N rows are mmsbm_scan_topn's
 * list for that N, bit for bit.  When *out_count > capacity the rows are `capacity` distinct hits,
 * which ones is not defined; call again with capacity >= *out_count.  Rows from
 * min(*out_count, capacity) on are not touched: no address past row capacity - 1 is ever formed.
 * capacity = 0 is a count-only call; out_scores and out_keys may then be NULL.
 * The rows are placed by integer means only (ballots, popcounts, a wave's staging buffer of 256
 * rows in LDS and one 64-bit atomic add per flush of it on a cursor in the workspace, which the
 * call zeroes on `stream`); no floating-point value is combined anywhere.
 * Checked before any device call: a NULL ctx, order, theta, pr or out_count, a NULL output array
 * with capacity > 0, a NaN or infinite threshold, capacity < 0, a bad sample, a bad known-key table
 * or a missing, misaligned or small workspace: MMSBM_ERR_INVALID; K outside [1, MMSBM_MAX_K],
 * P above 2 000 000 (the packed key) or an ensemble whose W tile exceeds the LDS (as for the census):
 * MMSBM_ERR_UNSUPPORTED.  P < 3: *out_count = 0.  The list itself has no cap but the caller's memory
 * (16 bytes per row).
 * ws: mmsbm_scan_above_workspace_bytes(ctx) bytes of device scratch, 16-byte aligned, the caller's;
 * its size follows the context's shape only.  theta and pr are only read; all launches go to
 * `stream` and nothing synchronises.  The environment variable MMSBM_SCAN_ABOVE_GRID=<workgroups>
 * overrides the grid (measurement; the set of rows does not depend on it).  Needs R >= 2.  Replaces
 * nothing in the reference. */
int mmsbm_scan_above_workspace_bytes(const mmsbm_ctx *ctx, int64_t *bytes);
int mmsbm_scan_above(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                     const double *theta, const double *pr, int32_t sample, double threshold,
                     int64_t capacity, void *ws, int64_t ws_bytes, double *out_scores,
                     int64_t *out_keys, int64_t *out_count, void *stream);

/* Pair-masked census and threshold scan: the two calls above with one more rule of eligibility, a
 * predicate on PAIRS of genes.  A key table cannot carry such a rule (a blocked pair is P - 2 keys);
 * a bit matrix can, and lets the sweep drop whole work items and tiles before any MFMA is issued.
 * mask: device uint32[P16][MW] in RANK POSITIONS (those of `order`), P16 = P rounded up to 16 (at
 * least 16) and MW = ceil(P16 / 32), as mmsbm_pair_mask_shape returns them (rows, words_per_row).
 * Bit y & 31 of mask[x][y >> 5] set means the pair of rank positions (x, y) is blocked.  Only x < y
 * is ever read: the lower triangle, the diagonal, rows >= P and bits >= P are ignored (the rows exist
 * so that no kernel needs a row guard).  A triple a < b < c is eligible when it is eligible for the
 * unmasked call and none of (a, b), (a, c), (b, c) is blocked.  The mask is the caller's and is only
 * read.
 * Everything else is the unmasked call's: the arguments, the results (out_counts[M] = the number of
 * masked-eligible triples; the threshold scan's always-full count, its arrival-order rows, no address
 * at or past row `capacity` formed), integer-only combination across lanes, the error codes, the
 * workspaces (mmsbm_census_workspace_bytes, mmsbm_scan_above_workspace_bytes) and the grid variables
 * (MMSBM_CENSUS_GRID, MMSBM_SCAN_ABOVE_GRID).  The score phase is not touched: a score carries the
 * bits the unmasked families give that triple, so a masked call with an all-zero mask returns what
 * the unmasked call returns, and a masked call returns what the unmasked call returns with the keys
 * of every triple that contains a blocked pair added to `known`.
 * P <= 16384 (the pair census's cap: a row of bits is at most 2 KiB of LDS, the mask 32 MiB); above
 * it the three calls return MMSBM_ERR_UNSUPPORTED.  A NULL mask is MMSBM_ERR_INVALID: the unmasked
 * call exists for that.  All checks come before any device call.  Replaces nothing in the
 * reference. */
int mmsbm_pair_mask_shape(const mmsbm_ctx *ctx, int32_t *rows, int32_t *words_per_row);
int mmsbm_scan_census_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                             int64_t n_known, const uint32_t *mask, const double *theta,
                             const double *pr, int32_t sample, const double *thresholds, int32_t M,
                             void *ws, int64_t ws_bytes, int64_t *out_counts, void *stream);
int mmsbm_scan_above_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                            int64_t n_known, const uint32_t *mask, const double *theta,
                            const double *pr, int32_t sample, double threshold, int64_t capacity,
                            void *ws, int64_t ws_bytes, double *out_scores, int64_t *out_keys,
                            int64_t *out_count, void *stream);

/* Vote scan: for every one of the scan's eligible triples, in how many of the scored slots (EM
 * restarts) its score is at or above one threshold; counted and listed.  A mean of 0.5 can be eight
 * restarts at 0.5 or four at 0.95 and four at 0.05: every other family reduces the batch to one score
 * per triple first and cannot tell.  order, known, n_known, theta, pr, sample, ws and stream mean what
 * they mean for mmsbm_scan_census, and a triple is eligible exactly as there (rank positions
 * a < b < c < P whose packed key is not among `known`).
 * The scored slots: the ns = active-prefix slots for sample = -1, that one slot (ns = 1) for
 * sample >= 0.  A slot's own score is the bits a single-sample call on that slot forms (the ensemble
 * path forms every slot's tile from zero with that call's MFMA chain before it adds them; the compare
 * sits there).  An eligible triple's votes = the number of scored slots whose own score is
 * >= threshold, in [0, ns].  A hit is an eligible triple with votes >= min_votes, 1 <= min_votes <= ns.
 * Result (device): out_hist int64[ns + 1], zeroed by the call on `stream` and always written:
 * out_hist[v] = the eligible triples with exactly v votes; its sum is mmsbm_scan_census's total, and
 * sum_v v out_hist[v] is the sum over the scored slots s of mmsbm_scan_census's count at `threshold`
 * for sample = s.  *out_count int64[1] = the number of hits, always the full number, also when it
 * exceeds `capacity`: the sum of out_hist[v] over v >= min_votes.  The first
 * min(*out_count, capacity) rows of out_scores f64[capacity], out_keys int64[capacity] and out_votes
 * int32[capacity] hold hits: the ensemble score (the slots' tiles added in slot order and divided by
 * ns: the bits mmsbm_scan_topn, the census and the threshold scan give that triple for the same
 * `sample`), the packed key (a P + b) P + c and the votes.  The rows are written exactly as
 * mmsbm_scan_above writes its rows: in ARRIVAL order, so that only the SET of rows is defined;
 * complete, each hit once, when *out_count <= capacity; `capacity` distinct hits otherwise; rows from
 * min(*out_count, capacity) on are not touched and no address at or past row `capacity` is ever
 * formed.  capacity = 0 is a histogram-only call; the three row arrays may then be NULL.  P < 3:
 * out_hist is all zeros and *out_count = 0.
 * Everything that crosses a lane or a workgroup is an integer (ballots, popcounts, LDS adds, one
 * 64-bit global add per workgroup and nonzero counter into out_hist, one 64-bit atomic add per flush
 * of a wave's staging buffer on a cursor in the workspace, which the call zeroes on `stream`; a
 * histogram-only call stages nothing and takes *out_count from out_hist); no
 * floating-point value is combined beyond the score phase's own fixed-order sums, so out_hist, the
 * set of rows and every row's bits do not depend on the grid, the batch the slots sit in or the
 * arrival order.
 * Checked before any device call: a NULL ctx, order, theta, pr, out_hist or out_count, a NULL row
 * array with capacity > 0, a NaN or infinite threshold, capacity < 0, min_votes outside [1, ns], a
 * bad sample, a bad known-key table or a missing, misaligned or small workspace: MMSBM_ERR_INVALID;
 * K outside [1, MMSBM_MAX_K], P above 2 000 000 (the packed key) or an ensemble whose W tile exceeds
 * the LDS (the census's rule and its 64 KiB): MMSBM_ERR_UNSUPPORTED.  The list has no cap but the
 * caller's memory (20 bytes per row).
 * ws: mmsbm_scan_votes_workspace_bytes(ctx) bytes of device scratch, 16-byte aligned, the caller's;
 * its size follows the context's shape only.  theta and pr are only read; all launches go to
 * `stream` and nothing synchronises.  The environment variable MMSBM_SCAN_VOTES_GRID=<workgroups>
 * overrides the grid (measurement; neither out_hist nor the set of rows depends on it).  Needs
 * R >= 2.  Replaces nothing in the reference. */
int mmsbm_scan_votes_workspace_bytes(const mmsbm_ctx *ctx, int64_t *bytes);
int mmsbm_scan_votes(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                     const double *theta, const double *pr, int32_t sample, double threshold,
                     int32_t min_votes, int64_t capacity, void *ws, int64_t ws_bytes,
                     int64_t *out_hist, double *out_scores, int64_t *out_keys, int32_t *out_votes,
                     int64_t *out_count, void *stream);

/* Quorum scan: the exact top N of the scan's eligible triples ranked by their m-th best restart
 * score, m = min_votes: the vote scan's consensus without a threshold chosen in advance.  order,
 * known, n_known, theta, pr, sample, N, ws, stream, eligibility, the packed key and the total order
 * (score descending; equal scores: smaller packed key first) are mmsbm_scan_topn's.
 * The scored slots and a slot's own score are the vote scan's: the ns = active-prefix slots for
 * sample = -1, that one slot (ns = 1) for sample >= 0; a slot's own score is the bits a single-sample
 * call on that slot forms.  The quorum score q_m of a triple is the m-th largest of those ns values,
 * 1 <= m <= ns: one of the slots' scores, bit for bit; no floating-point value is combined across
 * slots.  votes >= m at threshold t exactly when q_m >= t, so mmsbm_scan_votes' hits at (t, m) are
 * the triples with q_m >= t.  m = ns ranks by the minimum over the restarts, m = 1 by the maximum,
 * m = ns / 2 + 1 by the majority score.  With ns = 1 the list is mmsbm_scan_topn's for that sample,
 * bit for bit.
 * Result (device), as for mmsbm_scan_topn with q_m in out_scores: the first *out_count rows of
 * out_scores f64[N] and out_ids int32[N][3] hold the best triples under the total order;
 * *out_count < N when fewer are eligible (P < 3: 0); the tail is NaN / -1.  The list is unique: it
 * does not depend on the grid, the arrival order, the batch the slots sit in or the early exit below.
 * The kernel keeps, per tile element, a sorted list of depth D = min(m, ns - m + 1) in registers (the
 * D largest scores, or the D smallest when that list is no longer).  D <=
 * mmsbm_scan_quorum_max_depth() (4: every m for ns <= 8; the four lowest and the four highest m for
 * any ns); a deeper request is MMSBM_ERR_UNSUPPORTED.  Once more than ns - m slots of every element
 * of a tile score below the pruning bound in force, the tile's remaining slots are not formed: the
 * selection would have dropped every one of its elements.  The environment variable
 * MMSBM_SCAN_QUORUM_EARLY=0 turns that exit off and MMSBM_SCAN_QUORUM_GRID=<workgroups> lowers the
 * grid (measurement; the result depends on neither).
 * Checked before any device call: a NULL ctx, order, theta, pr, out_scores, out_ids or out_count,
 * N < 1, min_votes outside [1, ns], a bad sample, a bad known-key table or a missing, misaligned or
 * small workspace: MMSBM_ERR_INVALID; K outside [1, MMSBM_MAX_K], N above mmsbm_scan_max_n(), P above
 * 2 000 000, a depth above the cap or an ensemble whose W tile exceeds 64 KiB of LDS (the scan's
 * rule): MMSBM_ERR_UNSUPPORTED.
 * ws: mmsbm_scan_quorum_workspace_bytes(ctx, N) bytes of device scratch, 16-byte aligned, the
 * caller's; its size follows the context's shape and N only.  theta and pr are only read; all
 * launches go to `stream` and nothing synchronises.  Needs R >= 2.  Replaces nothing in the
 * reference. */
int mmsbm_scan_quorum_max_depth(void);
int mmsbm_scan_quorum_workspace_bytes(const mmsbm_ctx *ctx, int32_t N, int64_t *bytes);
int mmsbm_scan_quorum_topn(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                           const double *theta, const double *pr, int32_t sample, int32_t min_votes,
                           int32_t N, void *ws, int64_t ws_bytes, double *out_scores,
                           int32_t *out_ids, int64_t *out_count, void *stream);

/* Pair-masked pair census, vote scan and quorum scan: mmsbm_pair_census, mmsbm_scan_votes and
 * mmsbm_scan_quorum_topn with the pair mask of mmsbm_scan_census_masked behind n_known, under that
 * call's contract word for word.  mask: device uint32[P16][MW] in RANK POSITIONS, as
 * mmsbm_pair_mask_shape returns the shape; bit y & 31 of mask[x][y >> 5] set blocks the pair of rank
 * positions (x, y); only x < y is ever read; the mask is the caller's and is only read.  A triple
 * a < b < c is eligible when it is eligible for the unmasked call and none of (a, b), (a, c), (b, c)
 * is blocked.
 * Everything else is the unmasked call's: the arguments, the results (the pair matrix; out_hist, the
 * always-full *out_count, the arrival-order rows of which only the SET is defined, no address at or
 * past row `capacity` formed, rows from min(*out_count, capacity) on untouched; the quorum list under
 * the scan's total order with its NaN / -1 tail), integer-only combination across lanes, the error
 * codes, the grid and early-exit variables (MMSBM_PAIR_CENSUS_GRID, MMSBM_SCAN_VOTES_GRID,
 * MMSBM_SCAN_QUORUM_GRID, MMSBM_SCAN_QUORUM_EARLY) and the workspaces: the unmasked
 * mmsbm_pair_census_workspace_bytes, mmsbm_scan_votes_workspace_bytes and
 * mmsbm_scan_quorum_workspace_bytes size them, and none has grown.  The score phase is not touched: a
 * row's score, a slot's vote and q_m carry the bits the unmasked family gives that triple, so a masked
 * call with an all-zero mask returns what the unmasked call returns, and a masked call returns what
 * the unmasked call returns with the keys of every triple that contains a blocked pair added to
 * `known`.  What follows from that definition:
 *   - a blocked pair's row out_counts[x][y][.] of the pair matrix is zero (no eligible triple holds
 *     it), and for every m the sum of out_counts[x][y][m] over x < y is still three times
 *     mmsbm_scan_census_masked's count at thresholds[m] under the same mask;
 *   - out_hist sums to mmsbm_scan_census_masked's total (out_counts[M]) under the same mask;
 *   - votes >= m at threshold t exactly when the masked q_m >= t: mmsbm_scan_votes_masked's hits at
 *     (t, m) are the masked-eligible triples with q_m >= t, and the masked quorum list is the exact
 *     top N of q_m over the masked-eligible triples: its pruning bounds, the seeding pass's included,
 *     are formed from masked-eligible candidates only.
 * P <= 16384 (a row of bits is at most 2 KiB of LDS, the mask 32 MiB); above it the three calls
 * return MMSBM_ERR_UNSUPPORTED.  A NULL mask is MMSBM_ERR_INVALID: the unmasked call exists for that.
 * All checks come before any device call.  Replaces nothing in the reference. */
int mmsbm_pair_census_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                             int64_t n_known, const uint32_t *mask, const double *theta,
                             const double *pr, int32_t sample, const double *thresholds, int32_t M,
                             void *ws, int64_t ws_bytes, int32_t *out_counts, void *stream);
int mmsbm_scan_votes_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                            int64_t n_known, const uint32_t *mask, const double *theta,
                            const double *pr, int32_t sample, double threshold, int32_t min_votes,
                            int64_t capacity, void *ws, int64_t ws_bytes, int64_t *out_hist,
                            double *out_scores, int64_t *out_keys, int32_t *out_votes,
                            int64_t *out_count, void *stream);
int mmsbm_scan_quorum_topn_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                                  int64_t n_known, const uint32_t *mask, const double *theta,
                                  const double *pr, int32_t sample, int32_t min_votes, int32_t N,
                                  void *ws, int64_t ws_bytes, double *out_scores, int32_t *out_ids,
                                  int64_t *out_count, void *stream);

/* Pair vote census: the vote scan's counts binned by pair.  For one threshold, M vote levels and
 * every pair of rank positions x < y, the exact number of the scan's eligible triples that contain
 * both x and y and that at least levels[m] of the scored slots (EM restarts) score >= threshold: the
 * predicted, unmeasured interactions of a double-mutant query (x, y) that the restarts agree on,
 * where mmsbm_pair_census counts on their mean.  order, known, n_known, theta, pr, sample, ws, stream
 * and eligibility are mmsbm_scan_votes'; mmsbm_pair_votes_masked takes the pair mask behind n_known
 * under mmsbm_scan_votes_masked's rule (device uint32[P16][MW] in RANK POSITIONS; a triple with a
 * blocked pair is not eligible; a NULL mask is MMSBM_ERR_INVALID).
 * The scored slots are the vote scan's: the ns = active-prefix slots for sample = -1, that one slot
 * (ns = 1) for sample >= 0.  A slot's own score is the vote scan's too, the bits a single-sample call
 * on that slot forms, and a triple's votes = the number of scored slots whose own score is
 * >= threshold.
 * levels_host int32[M] on the HOST: non-decreasing (duplicates are fine), each in [1, ns],
 * 0 <= M <= mmsbm_pair_votes_max_m() (8).  The levels travel in the kernel's arguments by value (one
 * byte each): they need no device copy and no LDS table, and the array may be freed on return.
 * Result (device) out_counts int32[P][P][M] in rank positions, zeroed by the call on `stream`:
 * out_counts[x][y][m], x < y = the eligible triples that contain positions x and y and have votes
 * >= levels[m]; entries with x >= y stay 0.  A count is at most P - 2.  M = 0 writes nothing and
 * returns MMSBM_OK; P < 3: all 0.
 * Identities, exact:
 *   - for every m the sum of out_counts[x][y][m] over x < y is three times the sum over
 *     v >= levels[m] of mmsbm_scan_votes' out_hist[v] at the same threshold, sample and known keys
 *     (and, for the masked entry, of mmsbm_scan_votes_masked's under the same mask);
 *   - out_counts[.][.][m] is the scatter to their three pairs of mmsbm_scan_votes' hits at
 *     (threshold, min_votes = levels[m]); by the quorum scan's identity, the triples that contain the
 *     pair and have quorum score q_levels[m] >= threshold;
 *   - with ns = 1, levels = {1} gives mmsbm_pair_census at thresholds = {threshold}, word for word;
 *   - the masked entry with an all-zero mask returns the unmasked matrix; with a mask, the unmasked
 *     matrix with the keys of every triple that holds a blocked pair added to `known`; a blocked
 *     pair's entries are zero.
 * Everything that crosses a lane or a workgroup is an integer (ballots, popcounts, integer
 * cross-lane moves and relaxed agent-scope 32-bit atomic adds into out_counts), so the matrix does
 * not depend on the grid, the batch the slots sit in or the arrival order.
 * Checked before any device call: a NULL ctx, order, theta or pr, with M > 0 a NULL levels_host or
 * out_counts, a NaN or infinite threshold, a bad sample, a bad known-key table, a missing, misaligned
 * or small workspace, a level outside [1, ns] or below the one before it, M < 0, a NULL mask to the
 * masked entry: MMSBM_ERR_INVALID; M > 8, K outside [1, MMSBM_MAX_K], P > 16384 (the pair census's
 * cap) or an ensemble whose W tile exceeds the LDS (the census's rule and its 64 KiB):
 * MMSBM_ERR_UNSUPPORTED.
 * ws: mmsbm_pair_votes_workspace_bytes(ctx) bytes of device scratch, 16-byte aligned, the caller's;
 * its size follows the context's shape only.  theta and pr are only read; all launches go to
 * `stream` and nothing synchronises.  The environment variable MMSBM_PAIR_VOTES_GRID=<workgroups>
 * overrides the grid (measurement; the matrix does not depend on it).  Needs R >= 2.  Replaces
 * nothing in the reference. */
int mmsbm_pair_votes_max_m(void);
int mmsbm_pair_votes_workspace_bytes(const mmsbm_ctx *ctx, int64_t *bytes);
int mmsbm_pair_votes(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                     const double *theta, const double *pr, int32_t sample, double threshold,
                     const int32_t *levels_host, int32_t M, void *ws, int64_t ws_bytes,
                     int32_t *out_counts, void *stream);
int mmsbm_pair_votes_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                            int64_t n_known, const uint32_t *mask, const double *theta,
                            const double *pr, int32_t sample, double threshold,
                            const int32_t *levels_host, int32_t M, void *ws, int64_t ws_bytes,
                            int32_t *out_counts, void *stream);

/* Dispute scan: the exact top N of the scan's eligible triples ranked by the spread of their restart
 * scores: on which novel triples do the restarts disagree most.  order, known, n_known, theta, pr, N,
 * ws, stream, eligibility, the packed key and the total order (score descending; equal scores:
 * smaller packed key first) are mmsbm_scan_quorum_topn's, and so is the contract, word for word, with
 * the spread d_t in out_scores.
 * The scored slots are the ns = active-prefix slots; sample must be -1.  A slot's own score is the
 * vote scan's and the quorum scan's: the bits a single-sample call on that slot forms.  For a trim
 * t >= 0 with ns - 2 t >= 2 the spread of a triple is d_t = q_{1+t} - q_{ns-t}, q_m the quorum scan's
 * m-th largest slot score: t = 0 is the range max - min, t = 1 drops the single highest and the
 * single lowest restart, t = (ns - 2) / 2 on an even ns is the gap between the two middle scores.
 * d_t is one IEEE subtraction of two slot scores; nothing else is combined across slots; d_t >= +0.
 * Result (device), as for mmsbm_scan_quorum_topn: the first *out_count rows of out_scores f64[N] and
 * out_ids int32[N][3] hold the best triples under the total order; *out_count < N when fewer are
 * eligible (P < 3: 0); the tail is NaN / -1.  The list is unique: it does not depend on the grid, the
 * arrival order or the batch the slots sit in.
 * The kernel keeps, per tile element, two sorted lists of depth t + 1 in registers (the largest and
 * the smallest scores); t <= mmsbm_scan_spread_max_trim() (3: every legal trim for ns <= 9); a legal
 * trim above it is MMSBM_ERR_UNSUPPORTED.  Every slot of every tile is formed: a spread only grows as
 * slots arrive, so there is no early exit.  The environment variable
 * MMSBM_SCAN_SPREAD_GRID=<workgroups> lowers the grid (measurement; the result does not depend on it).
 * Checked before any device call: a NULL ctx, order, theta, pr, out_scores, out_ids or out_count,
 * N < 1, sample >= 0 or fewer than two active slots (one restart has no spread), trim < 0 or
 * ns - 2 trim < 2, a bad known-key table or a missing, misaligned or small workspace:
 * MMSBM_ERR_INVALID; K outside [1, MMSBM_MAX_K], N above mmsbm_scan_max_n(), P above 2 000 000, a legal
 * trim above the cap or an ensemble whose W tile exceeds 64 KiB of LDS (the scan's rule):
 * MMSBM_ERR_UNSUPPORTED.  Outputs and context are intact after a refusal.
 * ws: mmsbm_scan_spread_workspace_bytes(ctx, N) bytes of device scratch, 16-byte aligned, the
 * caller's; its size follows the context's shape and N only.  theta and pr are only read; all
 * launches go to `stream` and nothing synchronises.  Needs R >= 2.
 * mmsbm_scan_spread_topn_masked takes the pair mask of mmsbm_scan_census_masked behind n_known, under
 * mmsbm_scan_quorum_topn_masked's contract: the same workspace, P <= 16384 (MMSBM_ERR_UNSUPPORTED
 * above), a NULL mask MMSBM_ERR_INVALID; an all-zero mask returns the unmasked list, and a mask
 * returns the unmasked call's list with the keys of every triple that contains a blocked pair added
 * to `known`, bit for bit; the pruning bounds, the seeding pass's included, are formed from
 * masked-eligible candidates only.  Replaces nothing in the reference. */
int mmsbm_scan_spread_max_trim(void);
int mmsbm_scan_spread_workspace_bytes(const mmsbm_ctx *ctx, int32_t N, int64_t *bytes);
int mmsbm_scan_spread_topn(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known, int64_t n_known,
                           const double *theta, const double *pr, int32_t sample, int32_t trim,
                           int32_t N, void *ws, int64_t ws_bytes, double *out_scores,
                           int32_t *out_ids, int64_t *out_count, void *stream);
int mmsbm_scan_spread_topn_masked(mmsbm_ctx *ctx, const int32_t *order, const int64_t *known,
                                  int64_t n_known, const uint32_t *mask, const double *theta,
                                  const double *pr, int32_t sample, int32_t trim, int32_t N,
                                  void *ws, int64_t ws_bytes, double *out_scores, int32_t *out_ids,
                                  int64_t *out_count, void *stream);

/* Screen scan: for each query PAIR of genes, the score of Model.do_prediction (:530-547, no eps) of
 * every third gene, and the exact top N of them: what crossing the double-mutant query against the
 * array is predicted to find.  Notation as for mmsbm_partners_topn: order[P] (device) = the gene ids
 * sorted by str(id), Th' = theta in that order, p_1 the rating-1 lattice, a triple three rank
 * positions sorted ascending with the packed key (a P + b) P + c.
 * A query is two different gene ids; its rank positions are sorted to x < y (the order in which the
 * two ids are given does not matter).  A candidate is a third position c not in {x, y}; the triple is
 * {x, y, c} sorted, and its score factors through the two slots of p_1 the query fills:
 *   c < x:      S = v1 . Th'[c],  v1[i] = sum_j sum_k p_1[i][j][k] Th'[x][j] Th'[y][k]
 *   x < c < y:  S = v2 . Th'[c],  v2[j] = sum_i sum_k p_1[i][j][k] Th'[x][i] Th'[y][k]
 *   y < c:      S = v3 . Th'[c],  v3[k] = sum_i sum_j p_1[i][j][k] Th'[x][i] Th'[y][j]
 * (each v with the y slot contracted first, then the x slot, each contraction one fma chain over
 * ascending index: about 3 K^3 fma per query and sample; then a [Q][P] GEMM of inner size K).  The
 * triple's packed key increases with c across the three regions, so equal scores of one query order
 * by smaller c.
 * pairs_host int32[Q][2] (HOST) = gene ids in [0, P), the two of a row different; rows may repeat and
 * every row is answered on its own.  Q <= 65535; Q = 0 returns MMSBM_OK and writes nothing.  The ids
 * are copied to the workspace on `stream`.
 * Eligibility of c for the query (x, y): c < P and c not in {x, y}; c not in the query's known slice;
 * and, with a mask, none of (x, y), (x, c), (y, c) blocked (a query whose own pair is blocked has no
 * candidate).  Exclusion, per query in CSR form: known_off int64[Q + 1] (device) offsets into
 * known_thirds int32 (device), query i's slice holding the sorted, unique rank positions of the third
 * genes to skip; positions equal to x or y, or >= P, are ignored.  known_off = NULL: none.  mask: the
 * device uint32[P16][MW] bit matrix of mmsbm_pair_mask_shape in rank positions (bit y & 31 of
 * mask[x][y >> 5] blocks the pair x < y; only x < y is read), or NULL for none: this family has one
 * entry for both.  P <= 16384 when a mask is given.
 * sample >= 0 scores that slot of the active prefix; -1 the ensemble, formed as the scan forms it:
 * each slot's tile accumulated from zero, the tiles added in slot order, divided by n_active.
 * Nothing of a slot sits in LDS, so no ensemble size is refused.
 * mmsbm_screen_topn, result (device), row i for query i: the first out_count[i] rows of out_scores
 * f64[Q][N] and out_ids int32[Q][N][3] hold the query's best candidates under the scan's total order
 * (score descending; equal scores: the smaller packed key of the triple first); out_ids are the whole
 * triple's gene ids in key order, so a row can go straight into mmsbm_predict.  out_count int64[Q],
 * out_count[i] = min(N, the query's eligible candidates); the tail of a row is NaN / -1.  P < 3:
 * counts 0 and rows of NaN.  One workgroup sees a query's whole row: no merge, no published bound.
 * mmsbm_screen_scores, result (device): out f64[Q][P], out[i][c] = the score of query i with the
 * gene at RANK POSITION c, or NaN at every ineligible position (x and y included); otherwise exactly
 * the bits mmsbm_screen_topn ranks.
 * Every sum has a fixed order and no score is formed by an atomic: a query's scores and list depend
 * on (x, y), the sample and the eligibility only, not on Q, on the other queries, on the order in
 * which the pair's two ids were given, on the pass size or on the grid.  The scores need not equal
 * mmsbm_scan_topn's or mmsbm_partners_topn's bit for bit (the contraction order differs); they agree
 * to 1e-9 relative.
 * Refusals, all before any device call and with the outputs untouched.  MMSBM_ERR_INVALID: null
 * pointers; a bad sample; an id outside [0, P); a pair of equal ids; Q < 0 or Q > 65535; a missing,
 * misaligned or small workspace.  MMSBM_ERR_UNSUPPORTED: N outside [1, mmsbm_screen_max_n()] (1024: a
 * workgroup's candidate buffer stays in the LDS); K outside [1, MMSBM_MAX_K]; R < 2; P > 2 000 000
 * (the packed key); P > 16384 with a mask.
 * ws: mmsbm_screen_workspace_bytes(ctx, Q, N) bytes of device scratch, 16-byte aligned, the caller's
 * (N = 0: what mmsbm_screen_scores needs; a workspace for any N >= 1 serves it too); its size follows
 * the context's shape, Q and N only.  It holds the score rows of one pass: when Q rows of P16
 * doubles exceed 256 MiB the call runs passes over blocks of queries.  The environment variable
 * MMSBM_SCREEN_CHUNK=<queries per pass> lowers the block size (measurement and the tests of the pass
 * boundary; the results do not depend on it).  theta and pr are only read; all launches go to
 * `stream` and nothing synchronises.  The caller guarantees that order is a permutation of [0, P).
 * Replaces nothing in the reference. */
int mmsbm_screen_max_n(void);
int mmsbm_screen_workspace_bytes(const mmsbm_ctx *ctx, int64_t Q, int32_t N, int64_t *bytes);
int mmsbm_screen_topn(mmsbm_ctx *ctx, const int32_t *order, const int32_t *pairs_host, int64_t Q,
                      const int64_t *known_off, const int32_t *known_thirds, const uint32_t *mask,
                      const double *theta, const double *pr, int32_t sample, int32_t N, void *ws,
                      int64_t ws_bytes, double *out_scores, int32_t *out_ids, int64_t *out_count,
                      void *stream);
int mmsbm_screen_scores(mmsbm_ctx *ctx, const int32_t *order, const int32_t *pairs_host, int64_t Q,
                        const int64_t *known_off, const int32_t *known_thirds, const uint32_t *mask,
                        const double *theta, const double *pr, int32_t sample, void *ws,
                        int64_t ws_bytes, double *out, void *stream);

/* Screen statistics: a query pair's row, and the exact top N of it, by an order statistic of the
 * restarts' own scores instead of one slot or the mean: what mmsbm_scan_quorum_topn and
 * mmsbm_scan_spread_topn are genome-wide, per query pair.  Everything not said here (the queries, x < y,
 * the candidates c, the packed key, pairs_host, known_off / known_thirds, mask, Q, N, P, the outputs,
 * the workspace, MMSBM_SCREEN_CHUNK, the stream) is mmsbm_screen_topn's and mmsbm_screen_scores's.
 * Slots: the ns = n_active slots of the active prefix; there is no sample argument.  For a query
 * (x, y) and a position c, slot s's OWN SCORE is the word mmsbm_screen_scores(sample = s) writes at
 * [query][c], bit for bit: the same v vectors (screen_prep_kernel), the same MFMA chain from zero
 * over ascending k, each element keeping the chain of its own region.
 *   stat = MMSBM_SCREEN_STAT_QUORUM, arg = m in [1, ns]: the value is q_m, the m-th largest of the
 *     slots' own scores (m = 1: the maximum, m = ns: the minimum).  No floating-point value is combined
 *     across slots: the value is one slot's word, and with ns = 1, m = 1 the row is slot 0's row bit
 *     for bit.  At least m slots score c at or above T exactly when q_m >= T.
 *   stat = MMSBM_SCREEN_STAT_SPREAD, arg = the trim t >= 0 with ns - 2 t >= 2: the value is
 *     d_t = q_{1+t} - q_{ns-t}, ONE IEEE subtraction of two slot scores, so d_t >= +0 (t = 0: the
 *     range max - min).  Slots that agree bit for bit give +0 with the sign bit clear.
 * The kernel keeps, per element, the D largest and the D smallest scores in sorted lists held in
 * registers, D = min(m, ns - m + 1) for the quorum (the m-th largest is the (ns - m + 1)-th smallest:
 * the shorter list is read) and D = t + 1 for the spread; D <= mmsbm_screen_stat_max_depth() = 4, the
 * caps of mmsbm_scan_quorum_max_depth and mmsbm_scan_spread_max_trim.  Every slot of a row is formed
 * before anything is selected: there is no early exit.
 * Eligibility is exactly the screen scan's (c not in {x, y}; the query's known slice; the mask bits of
 * (x, y), (x, c), (y, c)); an ineligible place of a row is NaN and is no candidate of a list.
 * mmsbm_screen_stat_scores, result (device): out f64[Q][P] by RANK POSITION, as mmsbm_screen_scores.
 * mmsbm_screen_stat_topn, result (device): out_scores f64[Q][N], out_ids int32[Q][N][3], out_count
 * int64[Q] as mmsbm_screen_topn: the query's best N values under the screen scan's total order (value
 * descending; equal values by the smaller packed key of the sorted triple, i.e. smaller c first), the
 * tail NaN / -1; the scores are the words of the row.  Q = 0 returns MMSBM_OK and writes nothing;
 * P < 3: counts 0 and rows of NaN.
 * A row or a list depends on (x, y), the active slots and the eligibility only: not on Q, on the other
 * queries, on the order in which the pair's two ids were given, on the pass size or on the grid (every
 * chain has a fixed order, max and min are exact, no score is formed by an atomic).
 * Refusals, all before any device call and with the outputs untouched: those of mmsbm_screen_topn /
 * mmsbm_screen_scores (without the sample's), and MMSBM_ERR_INVALID: an unknown stat; m outside
 * [1, ns]; t < 0 or ns - 2 t < 2; the spread with ns < 2.  MMSBM_ERR_UNSUPPORTED: a legal argument
 * whose depth D exceeds mmsbm_screen_stat_max_depth().
 * ws: mmsbm_screen_workspace_bytes(ctx, Q, N) bytes, N = 0 for mmsbm_screen_stat_scores: the screen
 * scan's workspace, no larger.  Replaces nothing in the reference. */
#define MMSBM_SCREEN_STAT_QUORUM 0
#define MMSBM_SCREEN_STAT_SPREAD 1
int mmsbm_screen_stat_max_depth(void);
int mmsbm_screen_stat_topn(mmsbm_ctx *ctx, const int32_t *order, const int32_t *pairs_host, int64_t Q,
                           const int64_t *known_off, const int32_t *known_thirds,
                           const uint32_t *mask, const double *theta, const double *pr, int32_t stat,
                           int32_t arg, int32_t N, void *ws, int64_t ws_bytes, double *out_scores,
                           int32_t *out_ids, int64_t *out_count, void *stream);
int mmsbm_screen_stat_scores(mmsbm_ctx *ctx, const int32_t *order, const int32_t *pairs_host, int64_t Q,
                             const int64_t *known_off, const int32_t *known_thirds,
                             const uint32_t *mask, const double *theta, const double *pr,
                             int32_t stat, int32_t arg, void *ws, int64_t ws_bytes, double *out,
                             void *stream);

/* Partner statistics: the exact top N of a query gene's pairs by an order statistic of the restarts'
 * own scores instead of one slot or the mean: what mmsbm_scan_quorum_topn and mmsbm_scan_spread_topn
 * are genome-wide and mmsbm_screen_stat_topn is per query pair, per query gene.  Everything not said
 * here (queries_host, the candidates b < c of the query at q, the packed key of the sorted triple,
 * known_off / known_pairs, Q <= 65535, N <= mmsbm_partners_max_n(), the outputs with their NaN / -1
 * tail and out_count, MMSBM_PARTNERS_SELECT, the stream) is mmsbm_partners_topn's, and with a mask
 * mmsbm_partners_topn_masked's.  One entry serves both: mask = NULL means no mask, and P <= 16384
 * holds only when a mask is given.
 * Slots: the ns = n_active slots of the active prefix; there is no sample argument.  Slot s's OWN
 * SCORE of a candidate is the word mmsbm_partners_topn(sample = s) lists for it, bit for bit: the
 * same T tables (partners_prep_kernel), the same U / L rows, the same MFMA chain from zero over
 * ascending k, each lane keeping the chain of its own column (c < q: L, otherwise U) per slot, before
 * anything is inserted.
 *   stat = MMSBM_PARTNERS_STAT_QUORUM, arg = m in [1, ns]: the value is q_m, the m-th largest of the
 *     slots' own scores (m = 1: the maximum, m = ns: the minimum).  No floating-point value is
 *     combined across slots: the value is one slot's word, and with ns = 1, m = 1 the list is
 *     mmsbm_partners_topn(sample = 0)'s bit for bit.  At least m slots score the candidate at or above
 *     T exactly when q_m >= T.
 *   stat = MMSBM_PARTNERS_STAT_SPREAD, arg = the trim t >= 0 with ns - 2 t >= 2: the value is
 *     d_t = q_{1+t} - q_{ns-t}, ONE IEEE subtraction of two slot scores, so d_t >= +0 (t = 0: the
 *     range max - min).  Slots that agree bit for bit give +0 with the sign bit clear.
 * The kernel keeps, per element, sorted lists in registers of depth D = min(m, ns - m + 1) for the
 * quorum (the m-th largest is the (ns - m + 1)-th smallest: the shorter list is kept) and two of
 * depth D = t + 1 for the spread; D <= mmsbm_partners_stat_max_depth() = 4.
 * Exactness: no blocked or excluded candidate enters a candidate buffer, and every pruning bound (a
 * workgroup's N-th best, the query's published word) is formed from eligible candidates' final
 * statistic only, so it is a lower bound of the query's N-th best value.  A spread only grows as
 * slots arrive, so the spread forms every slot.  The quorum stops a wave's tile early: once more than
 * ns - m slots of EVERY element of the tile are strictly below the larger of the two bounds, no
 * element can reach it and the tile's remaining slots are not formed (wave-uniform; equal scores
 * stay in).  MMSBM_PARTNERS_STAT_EARLY=0 (read at the call) turns that off; the list depends on
 * neither setting.
 * Result (device): out_scores f64[Q][N], out_ids int32[Q][N][3], out_count int64[Q] as
 * mmsbm_partners_topn: the query's best N values under the scan's total order (value descending;
 * equal values by the smaller packed key of the sorted triple).  Q = 0 returns MMSBM_OK and writes
 * nothing; P < 3: counts 0 and rows of NaN.  A query's list and its words depend on the query, the
 * active slots and the eligibility only: not on Q, on the other queries, on the order of the slots,
 * on the grid or on the early exit (every chain has a fixed order, max and min are exact, no value
 * is formed by an atomic).
 * Refusals, all before any device call and with the outputs and the context untouched: those of
 * mmsbm_partners_topn (without the sample's), with a mask those of mmsbm_partners_topn_masked's mask
 * (P above 16384, a misaligned mask), and MMSBM_ERR_INVALID: an unknown stat; m outside [1, ns];
 * t < 0 or ns - 2 t < 2; the spread with ns < 2.  MMSBM_ERR_UNSUPPORTED: a legal argument whose depth
 * D exceeds mmsbm_partners_stat_max_depth(); the ensemble rule of the partner scan,
 * ns (4 ceil(K / 4) + 2) > 384.
 * ws: mmsbm_partners_workspace_bytes(ctx, Q, N) bytes: the partner scan's workspace, no larger.
 * Replaces nothing in the reference. */
#define MMSBM_PARTNERS_STAT_QUORUM 0
#define MMSBM_PARTNERS_STAT_SPREAD 1
int mmsbm_partners_stat_max_depth(void);
int mmsbm_partners_stat_topn(mmsbm_ctx *ctx, const int32_t *order, const int32_t *queries_host,
                             int64_t Q, const int64_t *known_off, const int64_t *known_pairs,
                             const uint32_t *mask, const double *theta, const double *pr, int32_t stat,
                             int32_t arg, int32_t N, void *ws, int64_t ws_bytes, double *out_scores,
                             int32_t *out_ids, int64_t *out_count, void *stream);

/* Link-sharded iteration (single sample over N ranks): each rank's context
 * holds 1/N of the train links (mmsbm_set_links) and the GLOBAL degree (mmsbm_set_degree).
 * Step 1, the accumulation half of make_iteration (:986-1012) over this rank's links:
 *   nth[B][P][K]   = per gene, the sum of its c-scaled responsibility marginals (theta not applied)
 *   S[B][R][K^3]   = the S lattice sums,  npr = p S.
 * The caller sums nth and S over ranks (one all-reduce of one buffer), then step 2 applies the
 * M-step (:1016-1028): theta <- theta nth / deg, p_r <- p_r S_r / (eps + sum_r p_r S_r).
 * Called on one rank with all links, the pair equals mmsbm_iterate(n = 1). */
int mmsbm_accumulate(mmsbm_ctx *ctx, const double *theta, const double *pr, double *nth, double *S,
                     void *stream);
int mmsbm_mstep(mmsbm_ctx *ctx, double *theta, double *pr, const double *nth, const double *S,
                void *stream);

/* Joint digenic + trigenic model (include/mmsbm_pairs.h): nth_add[B][P][K] (device; NULL = none)
 * is added to every gene's triplet sums before the division by the counter in mmsbm_iterate
 * (the pair loop's ntheta, :1608-1642 of src/TrigenicInteractionPredictor_23.py), and to nth in
 * mmsbm_accumulate.  The pointer is read at every launch; it stays set until replaced. */
int mmsbm_set_theta_addend(mmsbm_ctx *ctx, const double *nth_add);

/* Measurement: info[16] = observations, plan rows (3 streams on the small-K plans, stream 0 on the
 * large-K ones), stream-0 rows, stream-0 workgroups, stream-1/2 workgroups, S partials, partial
 * rows, most genes per stream-0 workgroup (per unit for the small-K plan), V tables computed per
 * iteration, stream-0 partial rows, 1 if the plan is the small-K one (K <= 12, sk.h; 2: with the
 * fused E-step launch, pass A then runs all three streams and pass B is empty; 0: the large-K
 * kernels), units (waves of work), [12] the compute-unit count the fused plan sized its units
 * from (0: the plan does not depend on it), [13] that plan's unit target, [14] Y entries of the
 * large-K plan (2 per observation), [15] the large-K gm_kernel's workgroups per S part for the
 * current active batch (1 or 2; it follows the batch, the bits do not: its X rows are formed in
 * two fixed halves either way; 0 on the small-K plans).  The fused plan's unit length, and so the
 * order of its sums, follows [12]: results are bitwise reproducible on one device model /
 * partition mode. */
int mmsbm_plan_info(const mmsbm_ctx *ctx, int32_t which, int64_t *info);

/* Kernel timing for measurement (bench.py): with stride n > 0, mmsbm_iterate records a HIP
 * event pair on the launch stream around every kernel of every n-th iteration (kernel ids:
 * 0 = pass A (large-K: stream 0 + Y entries; fused small-K: the whole E-step), 1 = the large-K
 * gene kernel (x0, S partials, Y sums) / the small-K pass B, 2 = fin (theta / p update));
 * 0 disables.  mmsbm_timing resets the counters; mmsbm_timing_result waits for the last event
 * and returns the summed device time (ms) and the number of timed launches of that kernel. */
int mmsbm_timing(mmsbm_ctx *ctx, int32_t stride);
int mmsbm_timing_result(mmsbm_ctx *ctx, int32_t kernel, double *total_ms, int64_t *count);

/* Measurement: n back-to-back launches of kernel `kernel` (ids as above) on the current theta /
 * pr, between one HIP event pair on `stream`; *avg_ms = elapsed / n.  The passes only read
 * theta / pr and fin runs in its sums-out mode into workspace scratch, so the parameters are
 * unchanged.  Synchronises the stream. */
int mmsbm_time_kernel(mmsbm_ctx *ctx, int32_t kernel, double *theta, double *pr, int32_t n,
                      void *stream, double *avg_ms);

#ifdef __cplusplus
}
#endif
#endif /* MMSBM_H */
