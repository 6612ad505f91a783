"""Genome-wide scan: the most probable trigenic interactions nobody has measured.

Host helpers of `EMEngine.scan_top` / `Model.predict_novel` (include/mmsbm.h, mmsbm_scan_topn) and
a small driver.  The helpers import without a GPU.

The reference keys a link by its three gene ids sorted as decimal strings
(src/TrigenicInteractionPredictor.py:349-358: '10' < '2' < '9'), and slots 1, 2, 3 of
pr[i][j][k] follow that order.  `rank_order(P)` is the gene ids in that order; a triple of distinct
genes is three positions a < b < c of it and its packed key is (a P + b) P + c.

    python -m trigenicinteractionpredictor_amd.scan -t train0.dat -e test0.dat -k 10 -n 8 -i 200 \
        --top 1000 [--exclude train,test|train|none] [--best] [--seed S] [-o novel.tsv]

fits the -n restarts as one batch for -i iterations (the initial states come from the same stdlib
`random` stream as `Model.initialize_parameters`, seeded once), scans once (the ensemble mean, or
with --best the restart of the highest train likelihood) and writes a TSV with the columns
rank, probability, ids, names.

With --gene NAME_OR_ID (repeatable, or a comma list; a name or an id as `do_prediction` takes them)
or --all-genes the driver asks the per-gene question instead (`EMEngine.partners_top`,
mmsbm_partners_topn): for each query gene its --top most probable partner pairs, as a TSV with the
columns query, rank, probability, ids, names, in query order and then by rank.

Two more tables come from the score census (`EMEngine.census`, mmsbm_scan_census), each written
next to the table above:
    --census FILE          threshold, count, fraction rows: how many eligible triples (those the scan
                           ranks under --exclude, scored by --best or the ensemble mean) have
                           P(r = 1) >= threshold; fraction = count / total, the total in a header
                           comment.  --thresholds LIST: a comma list of floats in (0, 1]; the default
                           is DEFAULT_THRESHOLDS: 0.99 0.95 0.9 0.8 0.7 0.6 0.5 0.4 0.3 0.2 0.1 0.05
                           0.02 0.01 0.005 0.002 0.001.  Rows go from the highest threshold down.
    --heldout-ranks FILE   (needs -e) one rank, probability, ids, real row per test link: its
                           genome-wide rank among every triple not trained on (1 + the number of
                           those scoring strictly above it), ordered by rank, equal ranks by key.

Two more come from the pair census (`EMEngine.pair_census`, mmsbm_pair_census), the census's counts
binned by pair: the question of a trigenic screen, whose unit of work is a double-mutant query crossed
against the whole array, is which pair to build next.
    --pairs FILE           the --top pairs of genes with the most eligible triples (under --exclude,
                           scored by --best or the ensemble mean) at or above --pair-threshold T
                           (default 0.5, in (0, 1]): rank, count, eligible, ids, names rows, best
                           first, equal counts by the pair's key; eligible = the pair's eligible
                           triples in all (P - 2 minus its measured ones).
    --gene-census FILE     one row per gene, in id order: gene, name and its count of eligible triples
                           at or above each of --thresholds (default DEFAULT_THRESHOLDS), from the
                           highest threshold down.

One more comes from the threshold scan (`EMEngine.scan_above`, mmsbm_scan_above), which lists what
the census counts: the predicted trigenic network at a probability cut.
    --network FILE         every eligible triple (under --exclude, scored by --best or the ensemble
                           mean) with P(r = 1) >= --network-threshold T (default 0.5, in (0, 1]), as
                           rank, probability, ids, names rows, best first, equal probabilities by key:
                           the main table's columns without the main table's cap.  Its row count is
                           the --census count at T.  More than --network-limit ROWS (default
                           10,000,000) of them is refused, with the count, before anything is
                           written.

One more comes from the vote scan (`EMEngine.vote_census` / `EMEngine.consensus`, mmsbm_scan_votes).
Every table above reduces the -n restarts to one score per triple first; EM restarts settle in
different optima, and a mean of 0.5 can be eight restarts at 0.5 or four at 0.95 and four at 0.05.
    --consensus FILE       per eligible triple (under --exclude), its votes: in how many of the -n
                           restarts its P(r = 1) is >= --consensus-threshold T (default 0.5, in
                           (0, 1]).  The header comments give `# samples`, `# threshold` and one
                           `# votes  v  count` line per v from -n down to 0: how many eligible triples
                           have exactly v votes.  Then rank, votes, probability, ids, names rows for
                           every triple with at least --min-votes M votes (in [1, -n]; default -n: the
                           restarts agree), by votes descending, then probability (the ensemble
                           mean, the main table's) descending, then key.  More than --consensus-limit
                           ROWS (default 10,000,000) of them is refused, with the count, before
                           anything is written.  Not with --best: one restart has nothing to vote on.

Two more come from the pair vote census (`EMEngine.pairs_consensus_top`, `EMEngine.gene_vote_census`,
mmsbm_pair_votes): --pairs and --gene-census counted on the restarts' votes, not on their mean.  A
pair can top --pairs on triples that half of the restarts reject.
    --pair-consensus FILE  the --top pairs of genes with the most eligible triples (under --exclude)
                           that at least --pair-votes M of the -n restarts score >= --pair-threshold
                           (M in [1, -n]; default -n: the restarts agree).  The header comments give
                           `# samples`, `# threshold` and `# min votes`; then --pairs' rows: rank,
                           count, eligible, ids, names.
    --gene-consensus FILE  one row per gene, in id order: gene, name and its count of eligible triples
                           with at least v votes at --pair-threshold, for every v from -n down to 1.
Not with --best: one restart has nothing to vote on.

One more comes from the quorum scan (`EMEngine.quorum_top`, mmsbm_scan_quorum_topn): the consensus
without a threshold chosen in advance.
    --quorum FILE          the --top eligible triples (under --exclude) ranked by their quorum score:
                           the M-th largest of the -n restarts' own P(r = 1), --quorum-votes M (in
                           [1, -n]; default -n: the minimum over the restarts, what all of them agree
                           on; 1: the maximum; -n / 2 + 1: the majority score).  A triple has at least
                           M votes at a threshold T (--consensus) exactly when its quorum score is
                           >= T.  The header comments give `# samples` and `# quorum votes`; then
                           rank, quorum, mean, min, max, ids, names rows, best first, equal quorum
                           scores by key.  mean, min and max are the listed triple's ensemble mean and
                           its lowest and highest restart score, from the predict kernel.  The kernel
                           keeps min(M, -n - M + 1) scores per triple, at most MAX_QUORUM_DEPTH = 4:
                           every M up to -n 8, the four lowest and the four highest M beyond.  Not
                           with --best: one restart has no quorum.

One more comes from the dispute scan (`EMEngine.spread_top`, mmsbm_scan_spread_topn): the opposite
question.  Every table above asks what the restarts agree on; this one asks where they disagree most,
which are the triples whose measurement would constrain the model most and the predictions to trust
least.
    --disputed FILE        the --top eligible triples (under --exclude) ranked by the spread of the -n
                           restarts' own P(r = 1): the (1 + T)-th largest minus the (1 + T)-th
                           smallest, --disputed-trim T (default 0: the range max - min; 1: without the
                           single highest and the single lowest restart, so that one stray restart
                           makes no dispute; T >= 0 must leave two scores, -n - 2 T >= 2, and is at
                           most MAX_SPREAD_TRIM = 3: every legal T up to -n 9).  The header comments
                           give `# samples` and `# disputed trim`; then rank, spread, mean, min, max,
                           ids, names rows, best first, equal spreads by key.  mean, min and max are
                           the listed triple's ensemble mean and its lowest and highest restart
                           score, from the predict kernel.  Not with --best and not with -n 1: one
                           restart has no spread.

Two options restrict every table they apply to by PAIRS of genes (scan.pair_mask and the masked
kernels, mmsbm_scan_topn_masked, mmsbm_scan_census_masked, mmsbm_scan_above_masked, ...): a triple
that contains a blocked pair is not eligible.
    --allow-genes FILE     one gene name or id per line: the gene universe, such as the strains of an
                           array.  Every pair that touches another gene is blocked.
    --block-pairs FILE     two gene names or ids per line, tab or space separated: these pairs are
                           blocked, such as the pairs known to interact digenically.
They apply to the main table (which then goes through `EMEngine.scan_top_any`: one masked top-N scan
up to 4096 rows), --census, --network, --screen (with --screen-quorum and --screen-disputed),
--disputed, --pair-consensus and --gene-consensus, and combine by OR.  With
--gene / --all-genes, --pairs, --gene-census, --consensus and --quorum, which the driver does not
restrict yet, they are refused.  --heldout-ranks is not restricted by them.

One more comes from the screen scan (`EMEngine.screen_top`, mmsbm_screen_topn): what crossing a
double-mutant query against the array is predicted to find.
    --screen FILE          per query pair of genes, its --screen-top N (default 20, in [1, 1024]) most
                           probable third genes among the eligible triples (under --exclude, scored by
                           --best or the ensemble mean): query, rank, probability, ids, names rows, in
                           query order and then by rank; query = the pair's two names.  The pairs come
                           from exactly one of --query-pairs FILE (the format of --block-pairs) and
                           --screen-best Q (the Q pairs --pairs ranks first at --pair-threshold, under
                           the same exclude and mask).  --allow-genes / --block-pairs apply to it.

Two more come from the screen scan's statistics (`EMEngine.screen_quorum_top`, `screen_spread_top`,
mmsbm_screen_stat_topn): --quorum and --disputed per query pair, over the query pairs of --query-pairs
or --screen-best and with the same --screen-top rows per pair.  Either goes with or without --screen.
    --screen-quorum FILE   per query pair, its --screen-top third genes ranked by their quorum score:
                           the M-th largest of the -n restarts' own P(r = 1), --screen-votes M (in
                           [1, -n]; default -n: the minimum over the restarts; the depth rule of
                           --quorum-votes).  A third gene has at least M votes at a threshold T exactly
                           when its quorum score is >= T.  The header comments give `# samples` and
                           `# screen votes`; then query, rank, quorum, mean, min, max, ids, names rows,
                           in query order and then by rank.
    --screen-disputed FILE per query pair, its --screen-top third genes ranked by the spread of the
                           -n restarts' own P(r = 1), --screen-trim T (default 0: max - min; the rule
                           of --disputed-trim).  The header comments give `# samples` and
                           `# screen trim`; then query, rank, spread, mean, min, max, ids, names rows.
mean, min and max are the listed triple's ensemble mean and its lowest and highest restart score, from
the predict kernel.  --exclude, --allow-genes and --block-pairs apply as they do to --screen.  Not
with --best (and --screen-disputed not with -n 1): one restart has no quorum and no spread.

Two more come from the partner scan's statistics (`EMEngine.partners_quorum_top`,
`partners_spread_top`, mmsbm_partners_stat_topn): --quorum and --disputed per query gene, over the
query genes of --gene / --all-genes (which they need) and with the same --top rows per gene.
    --partners-quorum FILE   per query gene, its --top partner pairs ranked by their quorum score, the
                             M-th largest of the -n restarts' own P(r = 1), --partners-votes M (in
                             [1, -n]; default -n; the depth rule of --quorum-votes).  The header
                             comments give `# samples` and `# partners votes`; then the --gene table's
                             rows with the quorum score in the probability's place: query, rank,
                             quorum, ids, names.
    --partners-disputed FILE per query gene, its --top partner pairs ranked by the spread of the -n
                             restarts' own P(r = 1), --partners-trim T (default 0: max - min; the rule
                             of --disputed-trim).  `# samples`, `# partners trim`; query, rank,
                             spread, ids, names rows.
--exclude applies as it does to the --gene table.  Not with --best (and --partners-disputed not with
-n 1); with --allow-genes / --block-pairs they are refused as --gene is (`EMEngine` takes the mask).

Exactness: the counts are exact for the scan's score bits.  A listed triple's probability comes from
the predict kernel, which sums in another order, so a triple within rounding distance (about 1e-12
relative) of another triple's score may be placed on either side of it.  (Listed triples are
compared with each other by their probabilities and never with their own scan score.)
"""
from __future__ import annotations

import getopt
import random
import sys

import numpy as np

SETS = ("train", "test")
MAX_TOP = 4096   # mmsbm_scan_max_n() (include/mmsbm.h): the largest N one scan returns
MAX_PARTNER_TOP = 1024   # mmsbm_partners_max_n(): the largest N per query gene
MAX_CENSUS_M = 1024      # mmsbm_census_max_m(): the most thresholds one census call takes
MAX_PAIR_CENSUS_M = 8    # mmsbm_pair_census_max_m(): the most thresholds one pair census call takes
MAX_PAIR_VOTES_M = 8     # mmsbm_pair_votes_max_m(): the most vote levels one pair vote census call takes
DEFAULT_PAIR_THRESHOLD = 0.5   # --pairs without --pair-threshold
DEFAULT_NETWORK_THRESHOLD = 0.5    # --network without --network-threshold
DEFAULT_NETWORK_LIMIT = 10000000   # --network without --network-limit: the most rows it writes
DEFAULT_CONSENSUS_THRESHOLD = 0.5    # --consensus without --consensus-threshold
DEFAULT_CONSENSUS_LIMIT = 10000000   # --consensus without --consensus-limit: the most rows it writes
MAX_SCREEN_TOP = 1024    # mmsbm_screen_max_n(): the largest N per query pair
DEFAULT_SCREEN_TOP = 20  # --screen without --screen-top: the rows per query pair
MAX_SCREEN_QUERIES = 65535   # the most query pairs one mmsbm_screen_topn call takes
MAX_QUORUM_DEPTH = 4     # mmsbm_scan_quorum_max_depth(): the deepest sorted list of the quorum scan
MAX_SPREAD_TRIM = 3      # mmsbm_scan_spread_max_trim(): the largest trim of the dispute scan
MAX_PARTNERS_STAT_DEPTH = 4  # mmsbm_partners_stat_max_depth(): the deepest sorted lists of the partner statistics
MAX_SCREEN_STAT_DEPTH = 4    # mmsbm_screen_stat_max_depth(): the deepest sorted lists of the screen statistics
DEFAULT_THRESHOLDS = (0.99, 0.95, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2, 0.1, 0.05, 0.02, 0.01, 0.005,
                      0.002, 0.001)   # --census without --thresholds


def rank_order(P: int) -> np.ndarray:
    """Gene ids 0..P-1 sorted by str(id): rank_order(12) = [0, 1, 10, 11, 2, ..., 9]."""
    return np.array(sorted(range(int(P)), key=str), dtype=np.int32)


def rank_of(order: np.ndarray) -> np.ndarray:
    """The inverse permutation: rank[id] = position of the id in `order`."""
    order = np.asarray(order)
    rank = np.empty(order.shape[0], dtype=np.int64)
    rank[order] = np.arange(order.shape[0], dtype=np.int64)
    return rank


def pack_keys(ids, rank, P: int) -> np.ndarray:
    """ids int[n][3] (gene ids) -> int64[n] packed keys (a P + b) P + c of their rank positions,
    each row's positions sorted ascending (a key's string-sorted ids already are)."""
    ids = np.asarray(ids, dtype=np.int64).reshape(-1, 3)
    pos = np.sort(np.asarray(rank, dtype=np.int64)[ids], axis=1)
    return (pos[:, 0] * int(P) + pos[:, 1]) * int(P) + pos[:, 2]


def _id_tables(source, exclude):
    if isinstance(source, (tuple, list)):   # (P, train ids, test ids); a table may be None
        P, tables = int(source[0]), dict(zip(SETS, source[1:]))
    else:                                   # a Model
        P, tables = int(source.P), {name: source._link_arrays(i)[0] for i, name in enumerate(SETS)
                                    if name in exclude}
    return P, [np.asarray(tables[name], dtype=np.int64).reshape(-1, 3) for name in exclude
               if tables.get(name) is not None]


def parse_exclude(text):
    """'train,test' | 'train' | 'test' | 'none' -> tuple of set names; ValueError otherwise."""
    if isinstance(text, (tuple, list)):
        names = tuple(text)
    else:
        names = () if text.strip() in ("", "none") else tuple(t.strip() for t in text.split(","))
    for n in names:
        if n not in SETS:
            raise ValueError("exclude: %r is none of train, test, none" % (n,))
    return tuple(dict.fromkeys(names))


def known_keys(source, exclude=SETS) -> np.ndarray:
    """Sorted, unique int64 packed keys of the measured triples of distinct genes: `source` is a
    Model or (P, train_ids, test_ids); keys with a repeated gene are dropped (never candidates)."""
    exclude = parse_exclude(exclude)
    P, tables = _id_tables(source, exclude)
    if not tables:
        return np.zeros(0, dtype=np.int64)
    ids = np.concatenate(tables, axis=0)
    distinct = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])
    return np.unique(pack_keys(ids[distinct], rank_of(rank_order(P)), P))


def partner_known(source, queries, exclude=SETS):
    """The measured partner pairs of each query gene, as mmsbm_partners_topn takes them:
    -> (known_off int64[Q + 1], known_pairs int64[known_off[Q]]), query i's slice holding the
    sorted, unique keys b P + c (rank positions b < c of the other two genes) of the measured
    triples of distinct genes that contain queries[i].  `source` is a Model or
    (P, train_ids, test_ids); `queries` are gene ids in [0, P) (IndexError otherwise)."""
    exclude = parse_exclude(exclude)
    P, tables = _id_tables(source, exclude)
    queries = np.asarray(queries, dtype=np.int64).reshape(-1)
    if queries.size and (queries.min() < 0 or queries.max() >= P):
        raise IndexError("query gene id outside [0, %d)" % P)
    off = np.zeros(queries.size + 1, dtype=np.int64)
    if not tables or not queries.size:
        return off, np.zeros(0, dtype=np.int64)
    ids = np.concatenate(tables, axis=0)
    distinct = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])
    rank = rank_of(rank_order(P))
    pos = np.sort(rank[ids[distinct]], axis=1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    # one (gene, pair of the other two) entry per slot of every triple, sorted by gene then pair
    both = np.unique(np.concatenate([a, b, c]) * (P * P) + np.concatenate([b * P + c, a * P + c, a * P + b]))
    who, pair = both // (P * P), both % (P * P)
    start = np.searchsorted(who, np.arange(P + 1))
    qpos = rank[queries]
    off[1:] = np.cumsum(start[qpos + 1] - start[qpos])
    pairs = np.concatenate([pair[start[q]:start[q + 1]] for q in qpos])
    return off, pairs.astype(np.int64)


def check_known_keys(known) -> np.ndarray:
    """The known-key table as the engine's scan families take it -> contiguous int64 (None: no
    keys); ValueError unless the keys are sorted and unique, as known_keys gives them."""
    known = np.zeros(0, np.int64) if known is None else np.ascontiguousarray(known, dtype=np.int64)
    if known.size > 1 and not (known[1:] > known[:-1]).all():
        raise ValueError("known keys must be sorted and unique (scan.known_keys)")
    return known


def check_partner_known(known, Q: int):
    """The partner scan's (known_off, known_pairs) for Q queries -> both as contiguous int64;
    ValueError unless the offsets are Q + 1 non-decreasing indices into the pairs and every query's
    slice is sorted and unique (a key may fall from one slice to the next), as partner_known gives
    them."""
    off = np.ascontiguousarray(known[0], dtype=np.int64).reshape(-1)
    pairs = np.ascontiguousarray(known[1], dtype=np.int64).reshape(-1)
    if off.size != Q + 1 or off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > pairs.size:
        raise ValueError("known offsets must be %d non-decreasing indices into the pair keys "
                         "(scan.partner_known)" % (Q + 1))
    rising = pairs[1:] > pairs[:-1]
    starts = off[1:-1]
    rising[starts[(starts > 0) & (starts < pairs.size)] - 1] = True   # a new query's slice
    if not rising[int(off[0]):max(int(off[-1]) - 1, int(off[0]))].all():
        raise ValueError("each query's known pair keys must be sorted and unique "
                         "(scan.partner_known)")
    return off, pairs


# -------------------------------------------------------------------------------- screen scan
def screen_pairs(pairs, P: int) -> np.ndarray:
    """Query pairs as mmsbm_screen_topn takes them -> contiguous int32[Q][2] gene ids; IndexError on
    an id outside [0, P), ValueError on a pair of one gene or rows that are not pairs."""
    pairs = np.asarray(pairs)
    if pairs.size and not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError("query pairs must be integer gene ids")
    if pairs.size % 2 or (pairs.ndim > 1 and pairs.shape[-1] != 2):
        raise ValueError("query pairs must be rows of two gene ids")
    pairs = np.ascontiguousarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.size and (pairs.min() < 0 or pairs.max() >= int(P)):
        raise IndexError("query gene id outside [0, %d)" % int(P))
    if (pairs[:, 0] == pairs[:, 1]).any():
        raise ValueError("a query pair needs two different genes")
    return pairs.astype(np.int32)


def screen_known(source, pairs, exclude=SETS):
    """The measured third genes of each query pair, as mmsbm_screen_topn takes them:
    -> (known_off int64[Q + 1], known_thirds int32[known_off[Q]]), query i's slice holding the
    sorted, unique rank positions of the third genes of the measured triples of distinct genes that
    contain both genes of pairs[i].  `source` is a Model or (P, train_ids, test_ids); `pairs` are
    gene ids in [0, P), two different ones per row (IndexError, ValueError otherwise)."""
    exclude = parse_exclude(exclude)
    P, tables = _id_tables(source, exclude)
    pairs = screen_pairs(pairs, P).astype(np.int64)
    Q = pairs.shape[0]
    off = np.zeros(Q + 1, dtype=np.int64)
    if not tables or not Q:
        return off, np.zeros(0, dtype=np.int32)
    ids = np.concatenate(tables, axis=0)
    distinct = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2])
    rank = rank_of(rank_order(P))
    pos = np.sort(rank[ids[distinct]], axis=1)
    a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]
    # one (pair key, third) entry per pair of every triple, sorted by pair then third
    both = np.unique(np.concatenate([a * P + b, a * P + c, b * P + c]) * P + np.concatenate([c, b, a]))
    who, third = both // P, both % P
    qpos = np.sort(rank[pairs], axis=1)
    qkey = qpos[:, 0] * P + qpos[:, 1]
    lo, hi = np.searchsorted(who, qkey, side="left"), np.searchsorted(who, qkey, side="right")
    off[1:] = np.cumsum(hi - lo)
    thirds = np.concatenate([third[l:h] for l, h in zip(lo, hi)])
    return off, thirds.astype(np.int32)


def check_screen_known(known, Q: int):
    """The screen scan's (known_off, known_thirds) for Q queries -> contiguous (int64, int32);
    ValueError unless the offsets are Q + 1 non-decreasing indices into the thirds and every query's
    slice is sorted and unique (a position may fall from one slice to the next), as screen_known
    gives them."""
    off = np.ascontiguousarray(known[0], dtype=np.int64).reshape(-1)
    thirds = np.ascontiguousarray(known[1], dtype=np.int32).reshape(-1)
    if off.size != Q + 1 or off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > thirds.size:
        raise ValueError("known offsets must be %d non-decreasing indices into the third genes "
                         "(scan.screen_known)" % (Q + 1))
    rising = thirds[1:] > thirds[:-1]
    starts = off[1:-1]
    rising[starts[(starts > 0) & (starts < thirds.size)] - 1] = True   # a new query's slice
    if not rising[int(off[0]):max(int(off[-1]) - 1, int(off[0]))].all():
        raise ValueError("each query's known third genes must be sorted and unique "
                         "(scan.screen_known)")
    return off, thirds


def screen_rows(id_gene, pairs, lists):
    """screen_top's lists for the query `pairs` (gene ids) -> the driver's rows [query, rank,
    probability, "i_j_k", names], in query order and then by rank; query = the pair's two names in
    the order of its key."""
    rows = []
    for (g1, g2), (scores, ids) in zip(pairs, lists):
        a, b = sorted((int(g1), int(g2)), key=str)
        query = "%s_%s" % (id_gene[a], id_gene[b])
        rows += [[query, i + 1, float(p), "_".join(str(int(x)) for x in row), sorted(id_gene[int(x)] for x in row)]
                 for i, (p, row) in enumerate(zip(scores, ids))]
    return rows


# ---------------------------------------------------------------------------------- pair mask
MAX_MASK_P = 16384   # the pair mask's cap on P (include/mmsbm.h, mmsbm_pair_mask_shape)


def pair_mask_shape(P: int):
    """(rows P16, words per row MW) of the pair mask of P genes, as mmsbm_pair_mask_shape returns
    them: P rounded up to 16 (at least 16) and ceil(P16 / 32); ValueError above MAX_MASK_P."""
    P = int(P)
    if not 0 <= P <= MAX_MASK_P:
        raise ValueError("pair mask: P=%d outside [0, %d]" % (P, MAX_MASK_P))
    P16 = max(16, (P + 15) // 16 * 16)
    return P16, (P16 + 31) // 32


def pair_mask(P: int, pairs=None, genes=None, matrix=None) -> np.ndarray:
    """The pair mask the masked scans take (include/mmsbm.h mmsbm_scan_census_masked): uint32
    [P16][MW] in RANK positions, bit y & 31 of mask[x][y >> 5] set = the pair of positions (x, y)
    is blocked, and a triple that contains a blocked pair is not eligible.  Three sources in GENE
    ids, combined by OR:
        pairs   int[n][2]: these pairs are blocked;
        genes   the allowed gene ids: every pair that touches another gene is blocked;
        matrix  bool[P][P]: an entry set on either side blocks the pair.
    Both triangles are written (the kernels read x < y only); the diagonal, rows >= P and bits >= P
    stay zero.  ValueError on an id outside [0, P) or a pair of one gene.  Goes through a bool
    [P16][P16] on the host."""
    P = int(P)
    P16, MW = pair_mask_shape(P)
    rank = rank_of(rank_order(P))
    blocked = np.zeros((P16, MW * 32), dtype=bool)

    def ids_of(a, what):
        a = np.asarray(a)
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise ValueError("pair mask: %s must be integer gene ids" % what)
        a = a.astype(np.int64)
        if a.size and (a.min() < 0 or a.max() >= P):
            raise ValueError("pair mask: %s hold a gene id outside [0, %d)" % (what, P))
        return a

    if pairs is not None:
        pairs = ids_of(pairs, "pairs").reshape(-1, 2)
        if (pairs[:, 0] == pairs[:, 1]).any():
            raise ValueError("pair mask: a pair of one gene")
        x, y = rank[pairs[:, 0]], rank[pairs[:, 1]]
        blocked[x, y] = True
        blocked[y, x] = True
    if genes is not None:
        out = np.ones(P, dtype=bool)
        out[rank[ids_of(genes, "genes").reshape(-1)]] = False    # in rank positions
        blocked[:P, :P] |= out[:, None] | out[None, :]
    if matrix is not None:
        matrix = np.asarray(matrix)
        if matrix.shape != (P, P):
            raise ValueError("pair mask: matrix must be bool[%d][%d]" % (P, P))
        m = matrix.astype(bool)
        m = m | m.T
        order = rank_order(P)
        blocked[:P, :P] |= m[order][:, order]      # position (x, y) <- genes (order[x], order[y])
    if P:
        blocked[np.arange(P), np.arange(P)] = False
    words = np.packbits(blocked, axis=1, bitorder="little").view("<u4")
    return np.ascontiguousarray(words.astype(np.uint32, copy=False))


def check_pair_mask(mask, P: int) -> np.ndarray:
    """The pair mask as the engine's masked calls take it -> the same contiguous uint32 array;
    ValueError unless it is uint32[P16][MW] (pair_mask_shape(P)) and C-contiguous, as pair_mask
    gives it.  Nothing is converted: a mask of another type or layout is a mistake."""
    P16, MW = pair_mask_shape(P)
    if not isinstance(mask, np.ndarray) or mask.dtype != np.uint32:
        raise ValueError("the pair mask must be a numpy uint32 array (scan.pair_mask)")
    if mask.shape != (P16, MW):
        raise ValueError("the pair mask must be uint32[%d][%d] for P=%d, not %r (scan.pair_mask)"
                         % (P16, MW, int(P), mask.shape))
    if not mask.flags.c_contiguous:
        raise ValueError("the pair mask must be C-contiguous (scan.pair_mask)")
    return mask


def read_allow_genes(path):
    """--allow-genes FILE -> the tokens, one name or id per line (blank lines and # comments skipped)."""
    with open(path, encoding="utf-8") as f:
        return [line.split()[0] for line in f if line.strip() and not line.lstrip().startswith("#")]


def read_block_pairs(path):
    """--block-pairs FILE -> [(token, token)], two names or ids per line, tab or space separated
    (blank lines and # comments skipped); ValueError on a line without exactly two."""
    out = []
    with open(path, encoding="utf-8") as f:
        for n, line in enumerate(f, 1):
            if not line.strip() or line.lstrip().startswith("#"):
                continue
            t = line.split()
            if len(t) != 2:
                raise ValueError("%s line %d: expected two genes" % (path, n))
            out.append((t[0], t[1]))
    return out


# ------------------------------------------------------------------------------------- census
def strict_thresholds(scores) -> np.ndarray:
    """The next double above each score: a census at them counts the triples scoring STRICTLY
    above each score (the census itself counts "at or above")."""
    return np.nextafter(np.asarray(scores, dtype=np.float64), np.inf)


def log_thresholds(lo: float, hi: float, n: int) -> np.ndarray:
    """n log-spaced thresholds from hi down to lo, both included (n = 1: hi alone); ValueError
    unless 0 < lo <= hi, both finite, and n >= 1."""
    lo, hi, n = float(lo), float(hi), int(n)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo <= hi) or n < 1:
        raise ValueError("log_thresholds needs 0 < lo <= hi and n >= 1")
    if n == 1:
        return np.array([hi])
    grid = np.geomspace(hi, lo, n)
    grid[0], grid[-1] = hi, lo      # the ends exactly
    return grid


def census_chunks(thresholds, max_m: int = MAX_CENSUS_M):
    """The binding's plan for any list of thresholds -> (chunks, perm): the thresholds sorted
    ascending (stable) and cut into float64 arrays of at most max_m, one census call each (no
    threshold: one empty chunk, the call that returns the total), and perm with
    sorted[i] = thresholds[perm[i]].  ValueError on a NaN or infinite threshold."""
    t = np.array(thresholds, dtype=np.float64).reshape(-1)
    if not np.isfinite(t).all():
        raise ValueError("census thresholds must be finite numbers")
    perm = np.argsort(t, kind="stable")
    ordered = np.ascontiguousarray(t[perm])
    step = max(int(max_m), 1)
    chunks = [ordered[i:i + step] for i in range(0, ordered.size, step)] or [ordered]
    return chunks, perm


def census_unsort(parts, perm) -> np.ndarray:
    """The chunks' counts (each int64[len(chunk)], in chunk order) -> int64 counts in the caller's
    order: out[perm[i]] = sorted count i."""
    perm = np.asarray(perm, dtype=np.int64)
    out = np.empty(perm.size, dtype=np.int64)
    if perm.size:
        out[perm] = np.concatenate([np.asarray(p, dtype=np.int64).reshape(-1) for p in parts])
    return out


def vote_level_chunks(levels, ns: int, max_m: int = MAX_PAIR_VOTES_M):
    """The binding's plan for any list of vote levels of the pair vote census -> (chunks, perm), as
    census_chunks plans thresholds: the levels sorted ascending (stable) and cut into int32 arrays of
    at most max_m, one mmsbm_pair_votes call each (no level: one empty chunk), and perm with
    sorted[i] = levels[perm[i]].  levels = None: 1..ns.  ValueError on a level that is no whole
    number or lies outside [1, ns], the scored slots, in EMEngine._vote_args' words."""
    ns = int(ns)
    raw = np.arange(1, ns + 1) if levels is None else np.array(levels).reshape(-1)
    if raw.size and (raw.dtype.kind not in "iuf" or not (np.isfinite(raw) & (raw == np.floor(raw))).all()):
        raise ValueError("vote levels must be whole numbers")
    lv = raw.astype(np.int64)
    for v in lv:
        if not 1 <= v <= ns:
            raise ValueError("min_votes %d outside [1, %d], the scored slots" % (v, ns))
    perm = np.argsort(lv, kind="stable")
    ordered = np.ascontiguousarray(lv[perm].astype(np.int32))
    step = max(int(max_m), 1)
    chunks = [ordered[i:i + step] for i in range(0, ordered.size, step)] or [ordered]
    return chunks, perm


# ----------------------------------------------------------------------------- threshold scan
class LimitError(ValueError):
    """A threshold scan would return more rows than its limit; nothing was launched for the list."""

    def __init__(self, count: int, limit: int):
        super().__init__("%d triples score at or above the threshold, more than the limit of %d rows: "
                         "raise the threshold or the limit" % (count, limit))
        self.count, self.limit = int(count), int(limit)


def bracket_threshold(n: int, hi: float, count_at, max_m: int = MAX_CENSUS_M) -> float:
    """The threshold scan_top_any fetches above: -> lo with count(lo) >= n, as close above n as
    censuses can bring it.  count_at(thresholds) -> the census's counts (scores >= each); `hi` is a
    score that at least one and fewer than n eligible triples reach unless scores tie (the last
    score of scan_top(max)); scores are probabilities, so count(0.0) is the eligible total.
    From (0.0, hi), each pass puts up to max_m evenly spaced thresholds strictly inside (lo, hi)
    and keeps the adjacent pair with count(lo') >= n > count(hi').  It stops when count(lo) <=
    n + max(n // 8, 4096), or when no double lies strictly between lo and hi: what then remains
    above n at lo are ties of the score next above lo.  Pure: no GPU, no state."""
    n, lo, hi = int(n), 0.0, float(hi)
    c_lo, c_hi = (int(c) for c in count_at(np.array([lo, hi])))
    if c_lo <= n or hi <= lo:       # everything
        return lo
    if c_hi >= n:                   # ties at hi reach rank n: nothing above hi holds n rows
        return hi
    while c_lo > n + max(n // 8, 4096):
        grid = np.unique(np.linspace(lo, hi, int(max_m) + 2)[1:-1])
        grid = grid[(grid > lo) & (grid < hi)]
        if not grid.size:           # adjacent doubles
            break
        counts = np.asarray(count_at(grid), dtype=np.int64)
        pts = np.concatenate([[lo], grid, [hi]])
        cnt = np.concatenate([[c_lo], counts, [c_hi]])
        j = int(np.flatnonzero(cnt >= n)[-1])       # counts do not increase with the threshold
        lo, c_lo, hi, c_hi = float(pts[j]), int(cnt[j]), float(pts[j + 1]), int(cnt[j + 1])
    return lo


def parse_unit_threshold(text, what: str) -> float:
    """'0.5' -> 0.5; ValueError unless it is one number in (0, 1].  `what` names the option's
    threshold in the message ("pair", "network")."""
    v = float(text)
    if not 0.0 < v <= 1.0:      # NaN fails the comparison
        raise ValueError("%s threshold outside (0, 1]" % what)
    return v


def network_rows(id_gene, scores, ids):
    """scan_above's arrays -> the main table's rows [rank, probability, "i_j_k", names]."""
    return [[i + 1, float(p), "_".join(str(int(g)) for g in row), sorted(id_gene[int(g)] for g in row)]
            for i, (p, row) in enumerate(zip(scores, ids))]


def pair_eligible(P: int, known=None, mask=None) -> np.ndarray:
    """int32 [P][P] in gene ids: the eligible triples of every pair of genes, P - 2 minus the number
    of `known` keys (sorted packed keys of rank positions, scan.known_keys) that contain the pair;
    the diagonal is zero.  Keys that pack no triple a < b < c < P are ignored, as the kernels ignore
    them.  mask: a pair mask (scan.pair_mask), read for x < y only as the kernels read it: a pair's
    eligible triples then are the third genes whose two pairs with it are unblocked (the product of
    the allowed matrix with itself), minus the known triples that the mask does not block already; a
    blocked pair has 0.  Pure numpy: the pair census never counts eligibility (an add per triple)."""
    P = int(P)
    allowed = None
    if mask is not None:
        bits = np.unpackbits(check_pair_mask(mask, P).view(np.uint8), axis=1, bitorder="little")[:P, :P]
        blocked = np.triu(bits.astype(bool), 1)
        allowed = ~(blocked | blocked.T)
        np.fill_diagonal(allowed, False)
        # float64 holds the counts exactly (at most P - 2) and multiplies through the BLAS
        count = allowed.astype(np.float64)
        pos = np.where(allowed, np.rint(count @ count).astype(np.int64), 0)     # in rank positions
    else:
        pos = np.full((P, P), max(P - 2, 0), dtype=np.int64)   # in rank positions
    if known is not None and len(known) and P >= 3:
        k = np.unique(np.asarray(known, dtype=np.int64).reshape(-1))
        k = k[(k >= 0) & (k < P ** 3)]
        a, b, c = k // (P * P), (k // P) % P, k % P
        ok = (a < b) & (b < c)
        if allowed is not None:     # a known triple with a blocked pair is gone already
            ok &= allowed[a, b] & allowed[a, c] & allowed[b, c]
        a, b, c = a[ok], b[ok], c[ok]
        for x, y in ((a, b), (a, c), (b, c)):
            np.subtract.at(pos, (x, y), 1)
            np.subtract.at(pos, (y, x), 1)
    np.fill_diagonal(pos, 0)
    rank = rank_of(rank_order(P))
    return pos[rank][:, rank].astype(np.int32)


def pair_key(i: int, j: int) -> str:
    """The pair's key as `links` spells keys: the ids in string order, joined by '_'."""
    return "_".join(sorted((str(int(i)), str(int(j)))))


def pair_rows(id_gene, counts, eligible, ids):
    """pairs_top's arrays -> rows [count, eligible, "i_j", [name1, name2]], names sorted."""
    return [[int(n), int(e), pair_key(i, j), sorted((id_gene[int(i)], id_gene[int(j)]))]
            for n, e, (i, j) in zip(counts, eligible, ids)]


def parse_thresholds(text):
    """'0.5,0.1' -> [0.5, 0.1]; ValueError when a token does not parse, the list is empty or a
    value lies outside (0, 1]."""
    values = [float(t) for t in text.split(",")]     # '' -> ValueError
    if not all(0.0 < v <= 1.0 for v in values):      # NaN fails the comparison
        raise ValueError("threshold outside (0, 1]")
    return values


def ranks_of(eng, ids, known, sample=None):
    """Listed triples ids int32[n][3] -> (probabilities f64[n] of the predict kernel for `sample`,
    or the mean over the active prefix added in slot order; ranks int64[n]): rank = 1 + the number
    of eligible triples (engine.census under `known`) scoring strictly above the probability.
    The listed triples that are eligible themselves are taken out of the census and compared with
    each other by their probabilities, so no triple is ever compared with its own scan score (whose
    last bits may differ from the predict kernel's)."""
    ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 3)
    known = np.zeros(0, np.int64) if known is None else np.asarray(known, dtype=np.int64)
    probs = eng.predict(ids)
    if sample is not None:
        p = probs[int(sample)]
    else:
        p = probs[0]
        for b in range(1, eng.active):
            p = p + probs[b]
        p = p / eng.active
    keys = pack_keys(ids, rank_of(rank_order(eng.P)), eng.P)
    own = (ids[:, 0] != ids[:, 1]) & (ids[:, 1] != ids[:, 2]) & (ids[:, 0] != ids[:, 2]) & ~np.isin(keys, known)
    own_keys, first = np.unique(keys[own], return_index=True)      # a triple listed twice counts once
    counts, _ = eng.census(strict_thresholds(p), np.union1d(known, own_keys), sample)
    own_p = np.sort(p[own][first])
    return p, counts + (own_p.size - np.searchsorted(own_p, p, side="right")) + 1


def heldout_rows(ids, counts, probs, ranks):
    """Test-link arrays and their ranks -> rows [rank, probability, "i_j_k", real] ordered by rank,
    equal ranks by key; real as Model.results has it (0 when the link has a rating-0 count)."""
    rows = [[int(r), float(p), "_".join(str(int(g)) for g in row), 0 if int(c[0]) else 1]
            for r, p, row, c in zip(ranks, probs, ids, counts)]
    rows.sort(key=lambda row: (row[0], row[2]))
    return rows


def resolve_genes(model, names):
    """Gene names or ids, as Model.do_prediction takes them, -> gene ids in [0, P): a token that
    reads as an integer is an id, anything else a name of the fold.  KeyError on an unknown name,
    IndexError on an id outside the table."""
    out = []
    for name in names:
        try:
            g = int(name)
        except ValueError:
            g = model.gene_id[name]
        if not 0 <= g < model.P:
            raise IndexError("gene id %d outside [0, %d)" % (g, model.P))
        out.append(g)
    return out


# ------------------------------------------------------------------------------------- driver
USAGE = """
Usage:
python -m trigenicinteractionpredictor_amd.scan [-h|--help] [-t|--train=] <train file>
    [-e|--test=] <test file> [-k|--k=] <number of groups> [-n|--num_samples=] <restarts>
    [-i|--num_iterations=] <EM iterations> [--seed=] <RNG seed> [--top=] <rows, default 100>
    [--exclude=] <train,test (default) | train | test | none> [--best] [-o|--out=] <TSV file>
    [--gene=] <gene name or id: its best partner pairs instead; repeatable, or a comma list>
    [--all-genes] <the best partner pairs of every gene>
    [--census=] <TSV file: counts of eligible triples at or above each threshold>
    [--thresholds=] <comma list of floats in (0, 1]; default 0.99 ... 0.001>
    [--heldout-ranks=] <TSV file: the genome-wide rank of every test link (needs -e)>
    [--pairs=] <TSV file: the --top gene pairs with the most eligible triples at or above T>
    [--pair-threshold=] <T, a float in (0, 1]; default 0.5>
    [--gene-census=] <TSV file: per gene, its eligible triples at or above each of --thresholds>
    [--pair-consensus=] <TSV file: the --top gene pairs with the most eligible triples that >= M restarts score >= --pair-threshold>
    [--pair-votes=] <M, an integer in [1, restarts]; default: all restarts>
    [--gene-consensus=] <TSV file: per gene, its eligible triples at every vote level at --pair-threshold>
    [--network=] <TSV file: every eligible triple at or above T, best first>
    [--network-threshold=] <T, a float in (0, 1]; default 0.5>
    [--network-limit=] <the most rows --network may write; default 10000000>
    [--consensus=] <TSV file: votes across the restarts; every eligible triple with >= M votes>
    [--consensus-threshold=] <T, a float in (0, 1]: a restart votes for a triple it scores >= T; default 0.5>
    [--min-votes=] <M, an integer in [1, restarts]; default: all restarts>
    [--consensus-limit=] <the most rows --consensus may write; default 10000000>
    [--quorum=] <TSV file: the --top eligible triples by their M-th best restart score>
    [--quorum-votes=] <M, an integer in [1, restarts]; default: all restarts (the minimum over them)>
    [--disputed=] <TSV file: the --top eligible triples by the spread of the restarts' scores>
    [--disputed-trim=] <T, an integer >= 0 with restarts - 2 T >= 2, at most 3; default 0 (max - min)>
    [--allow-genes=] <file, one gene name or id per line: only triples of these genes>
    [--block-pairs=] <file, two gene names or ids per line: no triple that contains such a pair>
    [--screen=] <TSV file: per query pair of genes, its most probable third genes>
    [--screen-top=] <rows per query pair, in [1, 1024]; default 20>
    [--query-pairs=] <file, two gene names or ids per line: the query pairs of --screen>
    [--screen-best=] <Q: the query pairs of --screen are the Q best of --pairs at --pair-threshold>
    [--screen-quorum=] <TSV file: per query pair, its --screen-top third genes by their M-th best restart score>
    [--screen-votes=] <M, an integer in [1, restarts]; default: all restarts (the minimum over them)>
    [--screen-disputed=] <TSV file: per query pair, its --screen-top third genes by the spread of the restarts' scores>
    [--screen-trim=] <T, an integer >= 0 with restarts - 2 T >= 2, at most 3; default 0 (max - min)>
    [--partners-quorum=] <TSV file: per query gene (--gene / --all-genes), its --top partner pairs by their M-th best restart score>
    [--partners-votes=] <M, an integer in [1, restarts]; default: all restarts (the minimum over them)>
    [--partners-disputed=] <TSV file: per query gene, its --top partner pairs by the spread of the restarts' scores>
    [--partners-trim=] <T, an integer >= 0 with restarts - 2 T >= 2, at most 3; default 0 (max - min)>
"""


def parse(argv):
    """Arguments -> cfg; cli.ArgError on a bad one (before anything touches a GPU).  -t, -e, -k, -n
    and -i are validated by cli.parse."""
    from . import cli
    cfg = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=SETS, best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
               pairs=None, pair_threshold=DEFAULT_PAIR_THRESHOLD, gene_census=None)
    # --network adds its three keys (network, network_threshold, network_limit, the latter two with
    # their defaults) only when one of its options is given: without them cfg is what it always was;
    # --consensus does the same with its four (consensus, consensus_threshold, min_votes,
    # consensus_limit) and --quorum with its two (quorum, quorum_votes); --allow-genes and
    # --block-pairs add their two (allow_genes, block_pairs) when one of them is given; --screen adds
    # its four (screen, screen_top, query_pairs, screen_best) in the same way, and --disputed its two
    # (disputed, disputed_trim); --screen-quorum and --screen-disputed add their two each
    # (screen_quorum, screen_votes; screen_disputed, screen_trim) and, being tables over --screen's
    # query pairs, --screen's four; --partners-quorum and --partners-disputed add their two each
    # (partners_quorum, partners_votes; partners_disputed, partners_trim); --pair-consensus,
    # --pair-votes and --gene-consensus add their three (pair_consensus, pair_votes, gene_consensus)
    try:
        opts, _ = getopt.getopt(argv, "ht:e:k:n:i:o:", ["help", "train=", "test=", "k=", "num_samples=",
                                                        "num_iterations=", "seed=", "top=", "exclude=",
                                                        "best", "out=", "gene=", "all-genes", "census=",
                                                        "thresholds=", "heldout-ranks=", "pairs=",
                                                        "pair-threshold=", "gene-census=", "network=",
                                                        "network-threshold=", "network-limit=", "consensus=",
                                                        "consensus-threshold=", "min-votes=",
                                                        "consensus-limit=", "quorum=", "quorum-votes=",
                                                        "allow-genes=", "block-pairs=", "screen=",
                                                        "screen-top=", "query-pairs=", "screen-best=",
                                                        "disputed=", "disputed-trim=", "screen-quorum=",
                                                        "screen-votes=", "screen-disputed=", "screen-trim=",
                                                        "partners-quorum=", "partners-votes=",
                                                        "partners-disputed=", "partners-trim=",
                                                        "pair-consensus=", "pair-votes=", "gene-consensus="])
    except getopt.GetoptError:
        print("Argument error. Aborting")
        raise cli.ArgError()
    for opt, arg in opts:
        if opt in ("-h", "--help"):
            print(USAGE)
            cfg["help"] = True
            return cfg
        try:
            if opt == "--top":
                if not 1 <= int(arg) <= MAX_TOP:
                    print("\n\nERROR: --top should be an integer number in [1, %d]" % MAX_TOP)
                    raise cli.ArgError()
                cfg["top"] = int(arg)
            elif opt == "--exclude":
                try:
                    cfg["exclude"] = parse_exclude(arg)
                except ValueError as e:
                    print("\n\nERROR: " + str(e))
                    raise cli.ArgError()
            elif opt == "--best":
                cfg["best"] = True
            elif opt == "--gene":
                names = [t.strip() for t in arg.split(",")]
                if not all(names):
                    print("\n\nERROR: --gene needs a gene name or id")
                    raise cli.ArgError()
                cfg["genes"] = cfg["genes"] + names
            elif opt == "--all-genes":
                cfg["all_genes"] = True
            elif opt == "--census":
                cfg["census"] = arg
            elif opt == "--heldout-ranks":
                cfg["heldout_ranks"] = arg
            elif opt == "--pairs":
                cfg["pairs"] = arg
            elif opt == "--gene-census":
                cfg["gene_census"] = arg
            elif opt == "--pair-threshold":
                try:
                    cfg["pair_threshold"] = parse_unit_threshold(arg, "pair")
                except ValueError:
                    print("\n\nERROR: --pair-threshold should be a number in (0, 1]")
                    raise cli.ArgError()
            elif opt == "--network":
                cfg["network"] = arg
            elif opt == "--network-threshold":
                try:
                    cfg["network_threshold"] = parse_unit_threshold(arg, "network")
                except ValueError:
                    print("\n\nERROR: --network-threshold should be a number in (0, 1]")
                    raise cli.ArgError()
            elif opt == "--network-limit":
                if not int(arg) >= 1:
                    print("\n\nERROR: --network-limit should be an integer number of rows >= 1")
                    raise cli.ArgError()
                cfg["network_limit"] = int(arg)
            elif opt == "--consensus":
                cfg["consensus"] = arg
            elif opt == "--consensus-threshold":
                try:
                    cfg["consensus_threshold"] = parse_unit_threshold(arg, "consensus")
                except ValueError:
                    print("\n\nERROR: --consensus-threshold should be a number in (0, 1]")
                    raise cli.ArgError()
            elif opt == "--min-votes":
                if not int(arg) >= 1:
                    print("\n\nERROR: --min-votes should be an integer number in [1, restarts (-n)]")
                    raise cli.ArgError()
                cfg["min_votes"] = int(arg)
            elif opt == "--consensus-limit":
                if not int(arg) >= 1:
                    print("\n\nERROR: --consensus-limit should be an integer number of rows >= 1")
                    raise cli.ArgError()
                cfg["consensus_limit"] = int(arg)
            elif opt == "--quorum":
                cfg["quorum"] = arg
            elif opt == "--quorum-votes":
                if not int(arg) >= 1:
                    print("\n\nERROR: --quorum-votes should be an integer number in [1, restarts (-n)]")
                    raise cli.ArgError()
                cfg["quorum_votes"] = int(arg)
            elif opt == "--disputed":
                cfg["disputed"] = arg
            elif opt == "--disputed-trim":
                if not int(arg) >= 0:
                    print("\n\nERROR: --disputed-trim should be an integer number >= 0")
                    raise cli.ArgError()
                cfg["disputed_trim"] = int(arg)
            elif opt == "--screen-quorum":
                cfg["screen_quorum"] = arg
            elif opt == "--screen-votes":
                if not int(arg) >= 1:
                    print("\n\nERROR: --screen-votes should be an integer number in [1, restarts (-n)]")
                    raise cli.ArgError()
                cfg["screen_votes"] = int(arg)
            elif opt == "--screen-disputed":
                cfg["screen_disputed"] = arg
            elif opt == "--screen-trim":
                if not int(arg) >= 0:
                    print("\n\nERROR: --screen-trim should be an integer number >= 0")
                    raise cli.ArgError()
                cfg["screen_trim"] = int(arg)
            elif opt == "--partners-quorum":
                cfg["partners_quorum"] = arg
            elif opt == "--partners-votes":
                if not int(arg) >= 1:
                    print("\n\nERROR: --partners-votes should be an integer number in [1, restarts (-n)]")
                    raise cli.ArgError()
                cfg["partners_votes"] = int(arg)
            elif opt == "--partners-disputed":
                cfg["partners_disputed"] = arg
            elif opt == "--partners-trim":
                if not int(arg) >= 0:
                    print("\n\nERROR: --partners-trim should be an integer number >= 0")
                    raise cli.ArgError()
                cfg["partners_trim"] = int(arg)
            elif opt == "--pair-consensus":
                cfg["pair_consensus"] = arg
            elif opt == "--pair-votes":
                if not int(arg) >= 1:
                    print("\n\nERROR: --pair-votes should be an integer number in [1, restarts (-n)]")
                    raise cli.ArgError()
                cfg["pair_votes"] = int(arg)
            elif opt == "--gene-consensus":
                cfg["gene_consensus"] = arg
            elif opt == "--allow-genes":
                cfg["allow_genes"] = arg
            elif opt == "--block-pairs":
                cfg["block_pairs"] = arg
            elif opt == "--screen":
                cfg["screen"] = arg
            elif opt == "--screen-top":
                if not 1 <= int(arg) <= MAX_SCREEN_TOP:
                    print("\n\nERROR: --screen-top should be an integer number in [1, %d]" % MAX_SCREEN_TOP)
                    raise cli.ArgError()
                cfg["screen_top"] = int(arg)
            elif opt == "--query-pairs":
                cfg["query_pairs"] = arg
            elif opt == "--screen-best":
                if not 1 <= int(arg) <= MAX_SCREEN_QUERIES:
                    print("\n\nERROR: --screen-best should be an integer number of pairs in [1, %d]"
                          % MAX_SCREEN_QUERIES)
                    raise cli.ArgError()
                cfg["screen_best"] = int(arg)
            elif opt == "--thresholds":
                try:
                    cfg["thresholds"] = parse_thresholds(arg)
                except ValueError:
                    print("\n\nERROR: --thresholds should be a comma list of numbers in (0, 1]")
                    raise cli.ArgError()
            elif opt == "--seed":
                cfg["seed"] = int(arg)
            elif opt in ("-o", "--out"):
                cfg["out"] = arg
            else:
                cfg = cli.parse([opt, arg], cfg)
        except ValueError:
            raise cli.ArgError()
    if any(key in cfg for key in ("network", "network_threshold", "network_limit")):
        cfg.setdefault("network", None)
        cfg.setdefault("network_threshold", DEFAULT_NETWORK_THRESHOLD)
        cfg.setdefault("network_limit", DEFAULT_NETWORK_LIMIT)
    if any(key in cfg for key in ("consensus", "consensus_threshold", "min_votes", "consensus_limit")):
        cfg.setdefault("consensus", None)
        cfg.setdefault("consensus_threshold", DEFAULT_CONSENSUS_THRESHOLD)
        cfg.setdefault("min_votes", cfg["samples"])     # every restart
        cfg.setdefault("consensus_limit", DEFAULT_CONSENSUS_LIMIT)
        if cfg["min_votes"] > cfg["samples"]:           # -n may come after --min-votes
            print("\n\nERROR: --min-votes should be an integer number in [1, restarts (-n)]")
            raise cli.ArgError()
        if cfg["consensus"] and cfg["best"]:
            print("\n\nERROR: --consensus counts votes across the restarts: it does not go with --best")
            raise cli.ArgError()
    if any(key in cfg for key in ("quorum", "quorum_votes")):
        cfg.setdefault("quorum", None)
        cfg.setdefault("quorum_votes", cfg["samples"])      # every restart
        if cfg["quorum_votes"] > cfg["samples"]:            # -n may come after --quorum-votes
            print("\n\nERROR: --quorum-votes should be an integer number in [1, restarts (-n)]")
            raise cli.ArgError()
        if quorum_depth(cfg["quorum_votes"], cfg["samples"]) > MAX_QUORUM_DEPTH:
            print("\n\nERROR: --quorum-votes %d of %d restarts: only the %d lowest and the %d highest values are "
                  "supported" % (cfg["quorum_votes"], cfg["samples"], MAX_QUORUM_DEPTH, MAX_QUORUM_DEPTH))
            raise cli.ArgError()
        if cfg["quorum"] and cfg["best"]:
            print("\n\nERROR: --quorum ranks by a score across the restarts: it does not go with --best")
            raise cli.ArgError()
    if any(key in cfg for key in ("disputed", "disputed_trim")):
        cfg.setdefault("disputed", None)
        cfg.setdefault("disputed_trim", 0)      # the range, max - min
        if cfg["samples"] < 2:                  # -n may come after --disputed-trim
            print("\n\nERROR: --disputed ranks by the spread across the restarts: it needs -n 2 or more")
            raise cli.ArgError()
        if cfg["disputed_trim"] not in spread_trims(cfg["samples"], None):
            print("\n\nERROR: --disputed-trim %d of %d restarts: the trim must leave two scores "
                  "(restarts - 2 T >= 2)" % (cfg["disputed_trim"], cfg["samples"]))
            raise cli.ArgError()
        if cfg["disputed_trim"] > MAX_SPREAD_TRIM:
            print("\n\nERROR: --disputed-trim %d: only trims up to %d are supported"
                  % (cfg["disputed_trim"], MAX_SPREAD_TRIM))
            raise cli.ArgError()
        if cfg["disputed"] and cfg["best"]:
            print("\n\nERROR: --disputed ranks by the spread across the restarts: it does not go with --best")
            raise cli.ArgError()
    if any(key in cfg for key in ("screen_quorum", "screen_votes")):
        cfg.setdefault("screen_quorum", None)
        cfg.setdefault("screen_votes", cfg["samples"])      # every restart
        cfg.setdefault("screen", None)                      # a table of --screen's query pairs: its checks below
        if cfg["screen_votes"] > cfg["samples"]:            # -n may come after --screen-votes
            print("\n\nERROR: --screen-votes should be an integer number in [1, restarts (-n)]")
            raise cli.ArgError()
        if quorum_depth(cfg["screen_votes"], cfg["samples"]) > MAX_SCREEN_STAT_DEPTH:
            print("\n\nERROR: --screen-votes %d of %d restarts: only the %d lowest and the %d highest values are "
                  "supported" % (cfg["screen_votes"], cfg["samples"], MAX_SCREEN_STAT_DEPTH, MAX_SCREEN_STAT_DEPTH))
            raise cli.ArgError()
        if cfg["screen_quorum"] and cfg["best"]:
            print("\n\nERROR: --screen-quorum ranks by a score across the restarts: it does not go with --best")
            raise cli.ArgError()
    if any(key in cfg for key in ("screen_disputed", "screen_trim")):
        cfg.setdefault("screen_disputed", None)
        cfg.setdefault("screen_trim", 0)        # the range, max - min
        cfg.setdefault("screen", None)
        if cfg["samples"] < 2:                  # -n may come after --screen-trim
            print("\n\nERROR: --screen-disputed ranks by the spread across the restarts: it needs -n 2 or more")
            raise cli.ArgError()
        if cfg["screen_trim"] not in spread_trims(cfg["samples"], None):
            print("\n\nERROR: --screen-trim %d of %d restarts: the trim must leave two scores "
                  "(restarts - 2 T >= 2)" % (cfg["screen_trim"], cfg["samples"]))
            raise cli.ArgError()
        if cfg["screen_trim"] > MAX_SCREEN_STAT_DEPTH - 1:
            print("\n\nERROR: --screen-trim %d: only trims up to %d are supported"
                  % (cfg["screen_trim"], MAX_SCREEN_STAT_DEPTH - 1))
            raise cli.ArgError()
        if cfg["screen_disputed"] and cfg["best"]:
            print("\n\nERROR: --screen-disputed ranks by the spread across the restarts: it does not go with --best")
            raise cli.ArgError()
    if any(key in cfg for key in ("partners_quorum", "partners_votes")):
        cfg.setdefault("partners_quorum", None)
        cfg.setdefault("partners_votes", cfg["samples"])    # every restart
        if cfg["partners_votes"] > cfg["samples"]:          # -n may come after --partners-votes
            print("\n\nERROR: --partners-votes should be an integer number in [1, restarts (-n)]")
            raise cli.ArgError()
        if quorum_depth(cfg["partners_votes"], cfg["samples"]) > MAX_PARTNERS_STAT_DEPTH:
            print("\n\nERROR: --partners-votes %d of %d restarts: only the %d lowest and the %d highest values are "
                  "supported" % (cfg["partners_votes"], cfg["samples"], MAX_PARTNERS_STAT_DEPTH,
                                 MAX_PARTNERS_STAT_DEPTH))
            raise cli.ArgError()
        if cfg["partners_quorum"] and cfg["best"]:
            print("\n\nERROR: --partners-quorum ranks by a score across the restarts: it does not go with --best")
            raise cli.ArgError()
    if any(key in cfg for key in ("partners_disputed", "partners_trim")):
        cfg.setdefault("partners_disputed", None)
        cfg.setdefault("partners_trim", 0)      # the range, max - min
        if cfg["samples"] < 2:                  # -n may come after --partners-trim
            print("\n\nERROR: --partners-disputed ranks by the spread across the restarts: it needs -n 2 or more")
            raise cli.ArgError()
        if cfg["partners_trim"] not in spread_trims(cfg["samples"], None):
            print("\n\nERROR: --partners-trim %d of %d restarts: the trim must leave two scores "
                  "(restarts - 2 T >= 2)" % (cfg["partners_trim"], cfg["samples"]))
            raise cli.ArgError()
        if cfg["partners_trim"] > MAX_PARTNERS_STAT_DEPTH - 1:
            print("\n\nERROR: --partners-trim %d: only trims up to %d are supported"
                  % (cfg["partners_trim"], MAX_PARTNERS_STAT_DEPTH - 1))
            raise cli.ArgError()
        if cfg["partners_disputed"] and cfg["best"]:
            print("\n\nERROR: --partners-disputed ranks by the spread across the restarts: it does not go with "
                  "--best")
            raise cli.ArgError()
    if any(key in cfg for key in ("pair_consensus", "pair_votes", "gene_consensus")):
        cfg.setdefault("pair_consensus", None)
        cfg.setdefault("pair_votes", cfg["samples"])    # every restart
        cfg.setdefault("gene_consensus", None)
        if cfg["pair_votes"] > cfg["samples"]:          # -n may come after --pair-votes
            print("\n\nERROR: --pair-votes should be an integer number in [1, restarts (-n)]")
            raise cli.ArgError()
        for name in ("pair_consensus", "gene_consensus"):
            if cfg[name] and cfg["best"]:
                print("\n\nERROR: --%s counts votes across the restarts: it does not go with --best"
                      % name.replace("_", "-"))
                raise cli.ArgError()
    if _partner_stat_tables(cfg) and not (cfg["genes"] or cfg["all_genes"]):
        print("\n\nERROR: --partners-quorum / --partners-disputed are tables per query gene: they need --gene or "
              "--all-genes")
        raise cli.ArgError()
    if any(key in cfg for key in ("allow_genes", "block_pairs")):
        cfg.setdefault("allow_genes", None)
        cfg.setdefault("block_pairs", None)
        for on, name in ((cfg["genes"], "--gene"), (cfg["all_genes"], "--all-genes"), (cfg["pairs"], "--pairs"),
                         (cfg["gene_census"], "--gene-census"), (cfg.get("consensus"), "--consensus"),
                         (cfg.get("quorum"), "--quorum")):
            if on:
                print("\n\nERROR: --allow-genes / --block-pairs restrict the main table, --census, --network, "
                      "--screen and --disputed: the driver does not apply them to %s" % name)
                raise cli.ArgError()
    if any(key in cfg for key in ("screen", "screen_top", "query_pairs", "screen_best")):
        cfg.setdefault("screen", None)
        cfg.setdefault("screen_top", DEFAULT_SCREEN_TOP)
        cfg.setdefault("query_pairs", None)
        cfg.setdefault("screen_best", None)
        if _screen_tables(cfg) and cfg["query_pairs"] is None and cfg["screen_best"] is None:
            print("\n\nERROR: --screen needs its query pairs: --query-pairs FILE or --screen-best Q")
            raise cli.ArgError()
        if cfg["query_pairs"] is not None and cfg["screen_best"] is not None:
            print("\n\nERROR: --query-pairs and --screen-best exclude each other")
            raise cli.ArgError()
    if cfg["genes"] and cfg["all_genes"]:
        print("\n\nERROR: --gene and --all-genes exclude each other")
        raise cli.ArgError()
    if (cfg["genes"] or cfg["all_genes"]) and cfg["top"] > MAX_PARTNER_TOP:
        print("\n\nERROR: with --gene / --all-genes --top should be in [1, %d]" % MAX_PARTNER_TOP)
        raise cli.ArgError()
    if cfg["heldout_ranks"] and "-e" not in [o for o, _ in opts] and "--test" not in [o for o, _ in opts]:
        print("\n\nERROR: --heldout-ranks needs a test file (-e)")
        raise cli.ArgError()
    return cfg


def _partner_stat_tables(cfg) -> bool:
    """Whether cfg asks for a statistic's table over query genes: --partners-quorum or --partners-disputed."""
    return bool(cfg.get("partners_quorum") or cfg.get("partners_disputed"))


def _screen_tables(cfg) -> bool:
    """Whether cfg asks for a table over query pairs: --screen, --screen-quorum or --screen-disputed."""
    return bool(cfg.get("screen") or cfg.get("screen_quorum") or cfg.get("screen_disputed"))


def partner_queries(model, cfg):
    """The driver's query gene ids (None: the genome-wide scan); cli.ArgError on a bad gene."""
    from . import cli
    if cfg.get("all_genes"):
        return list(range(model.P))
    if not cfg.get("genes"):
        return None
    try:
        return resolve_genes(model, cfg["genes"])
    except (KeyError, IndexError) as e:
        print("\n\nERROR: --gene: unknown gene %s" % (e,))
        raise cli.ArgError()


def driver_mask(model, cfg):
    """The driver's pair mask from --allow-genes / --block-pairs (None without them); cli.ArgError
    on a file that does not read or a gene the fold does not hold."""
    from . import cli
    if not (cfg.get("allow_genes") or cfg.get("block_pairs")):
        return None
    try:
        genes = pairs = None
        if cfg.get("allow_genes"):
            genes = resolve_genes(model, read_allow_genes(cfg["allow_genes"]))
        if cfg.get("block_pairs"):
            tokens = read_block_pairs(cfg["block_pairs"])
            flat = resolve_genes(model, [t for pair in tokens for t in pair])
            pairs = np.asarray(flat, dtype=np.int64).reshape(-1, 2)
        return pair_mask(model.P, pairs=pairs, genes=genes)
    except (KeyError, IndexError) as e:
        print("\n\nERROR: --allow-genes / --block-pairs: unknown gene %s" % (e,))
    except (OSError, ValueError) as e:
        print("\n\nERROR: --allow-genes / --block-pairs: %s" % (e,))
    raise cli.ArgError()


def screen_queries(model, cfg):
    """The driver's query pairs from --query-pairs, as int32[Q][2] gene ids (None: no --screen,
    --screen-quorum or --screen-disputed, or --screen-best, whose pairs come from the fit);
    cli.ArgError on a file that does not read, a line without two genes, a gene the fold does not
    hold, a pair of one gene or too many pairs."""
    from . import cli
    if not _screen_tables(cfg) or cfg.get("query_pairs") is None:
        return None
    try:
        tokens = read_block_pairs(cfg["query_pairs"])
        flat = resolve_genes(model, [t for pair in tokens for t in pair])
        pairs = screen_pairs(np.asarray(flat, dtype=np.int64).reshape(-1, 2), model.P)
        if pairs.shape[0] > MAX_SCREEN_QUERIES:
            raise ValueError("%d query pairs, more than %d" % (pairs.shape[0], MAX_SCREEN_QUERIES))
        return pairs
    except (KeyError, IndexError) as e:
        print("\n\nERROR: --query-pairs: unknown gene %s" % (e,))
    except (OSError, ValueError) as e:
        print("\n\nERROR: --query-pairs: %s" % (e,))
    raise cli.ArgError()


def screen_table(eng, model, cfg, known, sample, extras, queries, mask=None):
    """The driver's --screen table into `extras` (see run); queries: screen_queries' pairs, or None
    for --screen-best: the pairs pairs_top ranks first at --pair-threshold under the same exclude
    and mask.  --screen-quorum and --screen-disputed put their tables over the same pairs."""
    if not _screen_tables(cfg):
        return
    if queries is None:
        queries = eng.pairs_top(cfg["screen_best"], cfg["pair_threshold"], known, sample, **_masked(mask))[2]
    thirds = screen_known(model, queries, cfg["exclude"])
    if cfg.get("screen"):
        lists = eng.screen_top(queries, cfg["screen_top"], thirds, sample, mask=mask)
        extras["screen"] = screen_rows(model.id_gene, queries, lists)
    if cfg.get("screen_quorum"):
        lists = eng.screen_quorum_top(queries, cfg["screen_top"], cfg["screen_votes"], thirds, mask=mask)
        rows = screen_stat_rows(eng, model.id_gene, queries, lists)
        extras["screen_quorum"] = (eng.active, cfg["screen_votes"], rows)
    if cfg.get("screen_disputed"):
        lists = eng.screen_spread_top(queries, cfg["screen_top"], cfg["screen_trim"], thirds, mask=mask)
        rows = screen_stat_rows(eng, model.id_gene, queries, lists)
        extras["screen_disputed"] = (eng.active, cfg["screen_trim"], rows)


def screen_stat_rows(eng, id_gene, pairs, lists):
    """screen_quorum_top's or screen_spread_top's lists for the query `pairs` -> the driver's rows
    [query, rank, value, mean, min, max, "i_j_k", names], in query order and then by rank: per query
    quorum_rows' rows behind screen_rows' query name.  mean, min and max come from one predict call
    on every listed triple."""
    sizes = [len(scores) for scores, _ in lists]
    if not sum(sizes):
        return []
    listed = np.concatenate([ids for _, ids in lists if len(ids)])
    probs = np.asarray(eng.predict(listed)[:eng.active], dtype=np.float64)
    rows, at = [], 0
    for (g1, g2), (scores, ids), n in zip(pairs, lists, sizes):
        a, b = sorted((int(g1), int(g2)), key=str)
        query = "%s_%s" % (id_gene[a], id_gene[b])
        rows += [[query] + r for r in quorum_rows(id_gene, scores, ids, probs[:, at:at + n])]
        at += n
    return rows


def partner_stat_tables(eng, model, cfg, extras, queries):
    """The driver's --partners-quorum and --partners-disputed tables into `extras` (see run), over
    the query genes of --gene / --all-genes under the same --exclude as the partner table."""
    if not _partner_stat_tables(cfg) or queries is None:
        return
    known = partner_known(model, queries, cfg["exclude"])
    if cfg.get("partners_quorum"):
        lists = eng.partners_quorum_top(queries, cfg["top"], cfg["partners_votes"], known)
        extras["partners_quorum"] = (eng.active, cfg["partners_votes"], partner_rows(model.id_gene, queries, lists))
    if cfg.get("partners_disputed"):
        lists = eng.partners_spread_top(queries, cfg["top"], cfg["partners_trim"], known)
        extras["partners_disputed"] = (eng.active, cfg["partners_trim"], partner_rows(model.id_gene, queries, lists))


def partner_rows(id_gene, queries, lists):
    """partners_top's (or a partner statistic's) lists for the query genes -> the driver's rows
    [query, rank, value, "i_j_k", names], in query order and then by rank."""
    return [[id_gene[g], i + 1, float(p), "_".join(str(x) for x in row), sorted(id_gene[int(x)] for x in row)]
            for g, (scores, ids) in zip(queries, lists) for i, (p, row) in enumerate(zip(scores, ids))]


def _masked(mask):
    """The mask keyword of an engine call: nothing without a mask, so the unmasked calls are made
    as they always were."""
    return {} if mask is None else {"mask": mask}


def census_tables(eng, model, cfg, known, sample, extras, mask=None):
    """The driver's --census and --heldout-ranks tables into `extras` (see run); `known`: the
    keys --exclude names; `mask`: the pair mask of --allow-genes / --block-pairs (the census only)."""
    if cfg.get("census"):
        thresholds = sorted(cfg.get("thresholds") or DEFAULT_THRESHOLDS, reverse=True)
        counts, total = eng.census(thresholds, known, sample, **_masked(mask))
        extras["census"] = (thresholds, [int(c) for c in counts], total)
    if cfg.get("heldout_ranks"):
        ids, link_counts = model._link_arrays(1)
        probs, ranks = ranks_of(eng, ids, known_keys(model, ("train",)), sample)
        extras["heldout_ranks"] = heldout_rows(ids, link_counts, probs, ranks)


def pair_tables(eng, model, cfg, known, sample, extras):
    """The driver's --pairs and --gene-census tables into `extras` (see run)."""
    if cfg.get("pairs"):
        counts, eligible, ids = eng.pairs_top(cfg["top"], cfg["pair_threshold"], known, sample)
        extras["pairs"] = pair_rows(model.id_gene, counts, eligible, ids)
    if cfg.get("gene_census"):
        thresholds = sorted(cfg.get("thresholds") or DEFAULT_THRESHOLDS, reverse=True)
        counts = eng.gene_census(thresholds, known, sample)
        extras["gene_census"] = (thresholds, [model.id_gene[g] for g in range(model.P)], counts)


def pair_vote_tables(eng, model, cfg, known, extras, mask=None):
    """The driver's --pair-consensus and --gene-consensus tables into `extras` (see run); `mask`: the
    pair mask of --allow-genes / --block-pairs."""
    T = cfg.get("pair_threshold")
    if cfg.get("pair_consensus"):
        counts, eligible, ids = eng.pairs_consensus_top(cfg["top"], T, cfg["pair_votes"], known, **_masked(mask))
        extras["pair_consensus"] = (eng.active, T, cfg["pair_votes"], pair_rows(model.id_gene, counts, eligible, ids))
    if cfg.get("gene_consensus"):
        levels = list(range(eng.active, 0, -1))
        counts = eng.gene_vote_census(T, levels, known, **_masked(mask))
        extras["gene_consensus"] = (eng.active, T, levels, [model.id_gene[g] for g in range(model.P)], counts)


def network_table(eng, model, cfg, known, sample, extras, mask=None):
    """The driver's --network table into `extras` (see run); cli.ArgError when it would hold more
    rows than --network-limit."""
    from . import cli
    if not cfg.get("network"):
        return
    try:
        scores, ids = eng.scan_above(cfg["network_threshold"], known, sample, limit=cfg["network_limit"],
                                     **_masked(mask))
    except LimitError as e:
        eng.close()
        print("\n\nERROR: --network: %d triples have a probability of %r or more, above --network-limit %d: "
              "raise --network-threshold (or the limit)" % (e.count, cfg["network_threshold"], e.limit))
        raise cli.ArgError()
    extras["network"] = network_rows(model.id_gene, scores, ids)


def consensus_rows(id_gene, votes, scores, ids):
    """consensus's arrays -> rows [rank, votes, probability, "i_j_k", names]."""
    return [[i + 1, int(v), float(p), "_".join(str(int(g)) for g in row), sorted(id_gene[int(g)] for g in row)]
            for i, (v, p, row) in enumerate(zip(votes, scores, ids))]


def consensus_table(eng, model, cfg, known, extras):
    """The driver's --consensus table into `extras` (see run); cli.ArgError when it would hold more
    rows than --consensus-limit."""
    from . import cli
    if not cfg.get("consensus"):
        return
    T, M = cfg["consensus_threshold"], cfg["min_votes"]
    hist = eng.vote_census(T, known)
    try:
        votes, scores, ids = eng.consensus(T, M, known, limit=cfg["consensus_limit"])
    except LimitError as e:
        eng.close()
        print("\n\nERROR: --consensus: %d triples have a probability of %r or more in at least %d restarts, above "
              "--consensus-limit %d: raise --consensus-threshold or --min-votes (or the limit)"
              % (e.count, T, M, e.limit))
        raise cli.ArgError()
    extras["consensus"] = (eng.active, T, [int(c) for c in hist], consensus_rows(model.id_gene, votes, scores, ids))


def quorum_depth(votes: int, samples: int) -> int:
    """The scores the quorum scan keeps per triple for the votes-th largest of `samples`
    (EMEngine.quorum_depth): the shorter of the list from the top and the list from the bottom."""
    return min(int(votes), int(samples) - int(votes) + 1)


def quorum_rows(id_gene, scores, ids, probs):
    """quorum_top's arrays and predict's probs f64[samples][n] on those ids -> rows [rank, quorum
    score, mean, min, max, "i_j_k", names]; the mean is added in slot order."""
    if not len(scores):
        return []
    probs = np.asarray(probs, dtype=np.float64).reshape(-1, len(scores))
    mean = probs[0]
    for b in range(1, probs.shape[0]):
        mean = mean + probs[b]
    mean = mean / probs.shape[0]
    lo, hi = probs.min(axis=0), probs.max(axis=0)
    return [[i + 1, float(q), float(mean[i]), float(lo[i]), float(hi[i]), "_".join(str(int(g)) for g in row),
             sorted(id_gene[int(g)] for g in row)] for i, (q, row) in enumerate(zip(scores, ids))]


def quorum_table(eng, model, cfg, known, extras):
    """The driver's --quorum table into `extras` (see run)."""
    if not cfg.get("quorum"):
        return
    scores, ids = eng.quorum_top(cfg["top"], cfg["quorum_votes"], known)
    probs = eng.predict(ids)[:eng.active] if len(scores) else np.zeros((eng.active, 0))
    extras["quorum"] = (eng.active, cfg["quorum_votes"], quorum_rows(model.id_gene, scores, ids, probs))


def spread_trims(samples: int, cap=MAX_SPREAD_TRIM) -> list:
    """The trims the dispute scan takes for `samples` restarts (EMEngine.spread_trims): t >= 0 with
    samples - 2 t >= 2, up to `cap` (None: every legal one)."""
    legal = range(max(0, (int(samples) - 2) // 2 + 1)) if int(samples) >= 2 else range(0)
    return [t for t in legal if cap is None or t <= cap]


def spread_rows(id_gene, scores, ids, probs):
    """spread_top's arrays and predict's probs f64[samples][n] on those ids -> rows [rank, spread,
    mean, min, max, "i_j_k", names], formed as quorum_rows forms its rows."""
    return quorum_rows(id_gene, scores, ids, probs)


def spread_table(eng, model, cfg, known, extras, mask=None):
    """The driver's --disputed table into `extras` (see run)."""
    if not cfg.get("disputed"):
        return
    scores, ids = eng.spread_top(cfg["top"], cfg["disputed_trim"], known, **_masked(mask))
    probs = eng.predict(ids)[:eng.active] if len(scores) else np.zeros((eng.active, 0))
    extras["disputed"] = (eng.active, cfg["disputed_trim"], spread_rows(model.id_gene, scores, ids, probs))


def run(cfg, out=print, extras=None):
    """Fit the restarts as one batch, scan once, return the rows [rank, probability, ids, names]
    (with --gene / --all-genes: [query, rank, probability, ids, names], by query then rank).
    extras: a dict that receives "census" = (thresholds, counts, total) and "heldout_ranks" = rows
    when cfg asks for them (--census, --heldout-ranks), and "pairs" = rows [count, eligible, ids,
    names] and "gene_census" = (thresholds, names, counts int64[P][M]) for --pairs, --gene-census, and
    "network" = rows [rank, probability, ids, names] for --network, and "consensus" = (restarts,
    threshold, hist, rows [rank, votes, probability, ids, names]) for --consensus, and "quorum" =
    (restarts, votes, rows [rank, quorum score, mean, min, max, ids, names]) for --quorum, and
    "screen" = rows [query, rank, probability, ids, names] for --screen, and "disputed" = (restarts,
    trim, rows [rank, spread, mean, min, max, ids, names]) for --disputed, and "screen_quorum" =
    (restarts, votes, rows [query, rank, quorum score, mean, min, max, ids, names]) and
    "screen_disputed" = (restarts, trim, rows of the same form) for --screen-quorum and
    --screen-disputed, and "partners_quorum" = (restarts, votes, rows [query, rank, quorum score, ids,
    names]) and "partners_disputed" = (restarts, trim, rows of the same form) for --partners-quorum and
    --partners-disputed, and "pair_consensus" = (restarts, threshold, min votes, rows [count, eligible,
    ids, names]) and "gene_consensus" = (restarts, threshold, levels, names, counts int64[P][restarts])
    for --pair-consensus and --gene-consensus."""
    from .model import Model
    model = Model()
    model.get_traintest(cfg["train"], cfg["test"])
    queries = partner_queries(model, cfg)     # before anything touches a GPU
    mask = driver_mask(model, cfg)
    pair_queries = screen_queries(model, cfg)
    from . import _lib
    from .engine import EMEngine
    from .restarts import stream_states
    K, B = cfg["k"], cfg["samples"]
    if cfg["seed"] is not None:
        random.seed(cfg["seed"])
    eng = EMEngine(K, model.P, B=B, R=model.R, eps=model.eps)
    eng.set_links(_lib.SET_TRAIN, *model._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(model, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(cfg["iterations"])
    sample = int(np.argmax(eng.loglik(_lib.SET_TRAIN))) if cfg["best"] else None
    known = known_keys(model, cfg["exclude"])
    if extras is not None:
        census_tables(eng, model, cfg, known, sample, extras, mask)
        pair_tables(eng, model, cfg, known, sample, extras)
        pair_vote_tables(eng, model, cfg, known, extras, mask)
        network_table(eng, model, cfg, known, sample, extras, mask)
        consensus_table(eng, model, cfg, known, extras)
        quorum_table(eng, model, cfg, known, extras)
        screen_table(eng, model, cfg, known, sample, extras, pair_queries, mask)
        spread_table(eng, model, cfg, known, extras, mask)
        partner_stat_tables(eng, model, cfg, extras, queries)
    if queries is not None:
        out("partner pairs of %d genes: %s" % (len(queries), "sample %d" % sample if sample is not None
                                               else "mean of %d samples" % B))
        lists = eng.partners_top(queries, cfg["top"], partner_known(model, queries, cfg["exclude"]), sample)
        eng.close()
        return partner_rows(model.id_gene, queries, lists)
    out("scanning %d genes: %s" % (model.P, "sample %d" % sample if sample is not None
                                   else "mean of %d samples" % B))
    if mask is not None:    # the masked top-N scan; above its cap masked censuses and the masked threshold scan
        scores, ids = eng.scan_top_any(cfg["top"], known, sample, mask=mask)
    else:
        scores, ids = eng.scan_top(cfg["top"], known, sample)
    eng.close()
    return network_rows(model.id_gene, scores, ids)


def write_tsv(rows, stream, partners=False):
    if partners:
        stream.write("query\trank\tprobability\tids\tnames\n")
        for query, rank, p, key, names in rows:
            stream.write("%s\t%d\t%r\t%s\t%s\n" % (query, rank, p, key, "_".join(names)))
        return
    stream.write("rank\tprobability\tids\tnames\n")
    for rank, p, key, names in rows:
        stream.write("%d\t%r\t%s\t%s\n" % (rank, p, key, "_".join(names)))


def write_census_tsv(thresholds, counts, total, stream):
    stream.write("# total\t%d\n" % total)
    stream.write("threshold\tcount\tfraction\n")
    for t, c in zip(thresholds, counts):
        stream.write("%r\t%d\t%r\n" % (float(t), int(c), (int(c) / total) if total else 0.0))


def write_consensus_tsv(samples, threshold, hist, rows, stream):
    """hist[v], v = 0..samples: the eligible triples with exactly v votes, written from the most
    votes down."""
    stream.write("# samples\t%d\n" % samples)
    stream.write("# threshold\t%r\n" % float(threshold))
    for v in range(len(hist) - 1, -1, -1):
        stream.write("# votes\t%d\t%d\n" % (v, int(hist[v])))
    stream.write("rank\tvotes\tprobability\tids\tnames\n")
    for rank, votes, p, key, names in rows:
        stream.write("%d\t%d\t%r\t%s\t%s\n" % (rank, votes, p, key, "_".join(names)))


def write_quorum_tsv(samples, votes, rows, stream):
    stream.write("# samples\t%d\n" % samples)
    stream.write("# quorum votes\t%d\n" % votes)
    stream.write("rank\tquorum\tmean\tmin\tmax\tids\tnames\n")
    for rank, q, mean, lo, hi, key, names in rows:
        stream.write("%d\t%r\t%r\t%r\t%r\t%s\t%s\n" % (rank, q, mean, lo, hi, key, "_".join(names)))


def write_disputed_tsv(samples, trim, rows, stream):
    stream.write("# samples\t%d\n" % samples)
    stream.write("# disputed trim\t%d\n" % trim)
    stream.write("rank\tspread\tmean\tmin\tmax\tids\tnames\n")
    for rank, d, mean, lo, hi, key, names in rows:
        stream.write("%d\t%r\t%r\t%r\t%r\t%s\t%s\n" % (rank, d, mean, lo, hi, key, "_".join(names)))


def write_screen_stat_tsv(samples, arg, rows, stream, what):
    """The --screen-quorum (what = "quorum", arg = the votes) or --screen-disputed (what = "spread",
    arg = the trim) table."""
    stream.write("# samples\t%d\n" % samples)
    stream.write("# screen %s\t%d\n" % ("votes" if what == "quorum" else "trim", arg))
    stream.write("query\trank\t%s\tmean\tmin\tmax\tids\tnames\n" % what)
    for query, rank, v, mean, lo, hi, key, names in rows:
        stream.write("%s\t%d\t%r\t%r\t%r\t%r\t%s\t%s\n" % (query, rank, v, mean, lo, hi, key, "_".join(names)))


def write_partners_stat_tsv(samples, arg, rows, stream, what):
    """The --partners-quorum (what = "quorum", arg = the votes) or --partners-disputed (what =
    "spread", arg = the trim) table: the --gene table with the statistic in the probability's place."""
    stream.write("# samples\t%d\n" % samples)
    stream.write("# partners %s\t%d\n" % ("votes" if what == "quorum" else "trim", arg))
    stream.write("query\trank\t%s\tids\tnames\n" % what)
    for query, rank, v, key, names in rows:
        stream.write("%s\t%d\t%r\t%s\t%s\n" % (query, rank, v, key, "_".join(names)))


def write_pairs_tsv(rows, stream):
    stream.write("rank\tcount\teligible\tids\tnames\n")
    for i, (count, eligible, key, names) in enumerate(rows):
        stream.write("%d\t%d\t%d\t%s\t%s\n" % (i + 1, count, eligible, key, "_".join(names)))


def write_gene_census_tsv(thresholds, names, counts, stream):
    stream.write("gene\tname\t" + "\t".join("%r" % float(t) for t in thresholds) + "\n")
    for g, (name, row) in enumerate(zip(names, counts)):
        stream.write("%d\t%s\t%s\n" % (g, name, "\t".join("%d" % int(c) for c in row)))


def write_pair_consensus_tsv(samples, threshold, votes, rows, stream):
    stream.write("# samples\t%d\n" % samples)
    stream.write("# threshold\t%r\n" % float(threshold))
    stream.write("# min votes\t%d\n" % votes)
    write_pairs_tsv(rows, stream)


def write_gene_consensus_tsv(samples, threshold, levels, names, counts, stream):
    """counts[g][i]: gene g's eligible triples with at least levels[i] votes at the threshold."""
    stream.write("# samples\t%d\n" % samples)
    stream.write("# threshold\t%r\n" % float(threshold))
    stream.write("gene\tname\t" + "\t".join("%d" % int(v) for v in levels) + "\n")
    for g, (name, row) in enumerate(zip(names, counts)):
        stream.write("%d\t%s\t%s\n" % (g, name, "\t".join("%d" % int(c) for c in row)))


def write_heldout_tsv(rows, stream):
    stream.write("rank\tprobability\tids\treal\n")
    for rank, p, key, real in rows:
        stream.write("%d\t%r\t%s\t%d\n" % (rank, p, key, real))


def main(argv=None, out=print):
    from . import cli
    try:
        cfg = parse(sys.argv[1:] if argv is None else argv)
    except cli.ArgError:
        return 2
    if cfg.get("help"):
        return 0
    extras = {}
    try:
        rows = run(cfg, out, extras)
    except cli.ArgError:
        return 2
    if "census" in extras:
        with open(cfg["census"], "w", encoding="utf-8") as f:
            write_census_tsv(*extras["census"], f)
    if "heldout_ranks" in extras:
        with open(cfg["heldout_ranks"], "w", encoding="utf-8") as f:
            write_heldout_tsv(extras["heldout_ranks"], f)
    if "pairs" in extras:
        with open(cfg["pairs"], "w", encoding="utf-8") as f:
            write_pairs_tsv(extras["pairs"], f)
    if "gene_census" in extras:
        with open(cfg["gene_census"], "w", encoding="utf-8") as f:
            write_gene_census_tsv(*extras["gene_census"], f)
    if "pair_consensus" in extras:
        with open(cfg["pair_consensus"], "w", encoding="utf-8") as f:
            write_pair_consensus_tsv(*extras["pair_consensus"], f)
    if "gene_consensus" in extras:
        with open(cfg["gene_consensus"], "w", encoding="utf-8") as f:
            write_gene_consensus_tsv(*extras["gene_consensus"], f)
    if "network" in extras:
        with open(cfg["network"], "w", encoding="utf-8") as f:
            write_tsv(extras["network"], f)
    if "consensus" in extras:
        with open(cfg["consensus"], "w", encoding="utf-8") as f:
            write_consensus_tsv(*extras["consensus"], f)
    if "quorum" in extras:
        with open(cfg["quorum"], "w", encoding="utf-8") as f:
            write_quorum_tsv(*extras["quorum"], f)
    if "screen" in extras:
        with open(cfg["screen"], "w", encoding="utf-8") as f:
            write_tsv(extras["screen"], f, partners=True)
    if "disputed" in extras:
        with open(cfg["disputed"], "w", encoding="utf-8") as f:
            write_disputed_tsv(*extras["disputed"], f)
    if "screen_quorum" in extras:
        with open(cfg["screen_quorum"], "w", encoding="utf-8") as f:
            write_screen_stat_tsv(*extras["screen_quorum"], f, "quorum")
    if "screen_disputed" in extras:
        with open(cfg["screen_disputed"], "w", encoding="utf-8") as f:
            write_screen_stat_tsv(*extras["screen_disputed"], f, "spread")
    if "partners_quorum" in extras:
        with open(cfg["partners_quorum"], "w", encoding="utf-8") as f:
            write_partners_stat_tsv(*extras["partners_quorum"], f, "quorum")
    if "partners_disputed" in extras:
        with open(cfg["partners_disputed"], "w", encoding="utf-8") as f:
            write_partners_stat_tsv(*extras["partners_disputed"], f, "spread")
    partners = bool(cfg["genes"] or cfg["all_genes"])
    if cfg["out"]:
        with open(cfg["out"], "w", encoding="utf-8") as f:
            write_tsv(rows, f, partners)
    else:
        write_tsv(rows, sys.stdout, partners)
    return 0


if __name__ == "__main__":
    sys.exit(main())
