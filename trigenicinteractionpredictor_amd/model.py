"""`Model` — drop-in for the reference class `Model`
(AleixMT/TrigenicInteractionPredictor, src/TrigenicInteractionPredictor.py:33).

Same attribute names, method names, argument meaning and error behaviour.
The EM hot path (`make_iteration` :984-1043, `compute_likelihood` :952-974)
and the bulk test-set prediction (`do_prediction` :530-547 as used by
`calculate_test_set_results` :557-569) run as HIP kernels through
libmmsbm.so; there is no CPU fallback.  Ingestion, RNG initialisation, fold
splitting and text output stay on the host, as in the reference.

`theta` and `pr` are materialised as the reference's nested Python lists on
first access after the device moved them on; handing the lists out marks the
device copy stale, so in-place edits are uploaded before the next iteration
(the reference's `to_string`/`do_prediction` read them directly).
"""
from __future__ import annotations

import codecs
import random
import re

import numpy as np

from . import _lib
from .layout import links_to_arrays
from .tracked import TrackedLinks, tracked, version_of


NATIVE_INGEST = True   # get_traintest's native reader for canonical files (ingest.py)


def _masked(mask):
    """The mask keyword of an engine call: nothing without a mask, so the unmasked calls are made
    as they always were."""
    return {} if mask is None else {"mask": mask}


class Model:
    def __init__(self, device=None):
        self._links_version = 0
        self._fold = None               # native parse backing the lazy link dicts (ingest.py)
        self._fold_v = [None, None]     # table version that still equals the parsed arrays
        self.ntheta = []
        self._theta = []
        self.id_gene = {}
        self.gene_id = {}
        self._pr = []
        self.npr = []
        self.nlinks = {}
        self.links = {}
        self.test_links = {}
        self.results = []
        self.uniqueg = {}
        self.likelihood = 0
        self.heldoutlikelihood = 0
        self.vlikelihood = []
        self.R = 2
        self.K = 0
        self.P = 0
        self.eps = 1e-10
        self._device = device
        self._engine = None
        self._engine_key = None
        self._host_fresh = True   # host lists hold the newest parameters
        self._dev_fresh = False   # device tensors hold the newest parameters

    # ------------------------------------------------------------------ state
    def _pull(self):
        if self._host_fresh:
            return
        th, pr = self._engine.download()
        self._theta = th[0].tolist()
        self._pr = pr[0].tolist()
        self._host_fresh = True

    @property
    def theta(self):
        self._pull()
        self._dev_fresh = False   # the caller may edit the lists in place
        return self._theta

    @theta.setter
    def theta(self, value):
        self._pull()
        self._theta = value
        self._dev_fresh = False

    @property
    def pr(self):
        self._pull()
        self._dev_fresh = False
        return self._pr

    @pr.setter
    def pr(self, value):
        self._pull()
        self._pr = value
        self._dev_fresh = False

    # ---------------------------------------------- link tables (lazy after a native parse)
    # After get_traintest's native reader, `links` / `nlinks` / `test_links` are built as the
    # reference's dicts on first access; until then the engine reads the parsed arrays.  The
    # tables are TrackedLinks (tracked.py): every in-place edit (`links[k][r] += 1`,
    # `links[k] = [..]`, `del links[k]`, ...) changes their version, and so does assigning a new
    # table.  The device copy is rebuilt whenever the versions differ from the ones it was built
    # from, as the reference re-reads the dicts on every call (:987, :959).
    @property
    def links(self):
        if self._links is None:
            self._links = TrackedLinks(self._fold.links_dict())
            self._fold_v[0] = self._links.version.n
        return self._links

    @links.setter
    def links(self, value):
        # a plain dict is aliased, not copied (tracked.TrackedLinks): `m.links = d` then
        # `d[k][r] += 1` reaches the device like the reference's shared object would
        self._links = tracked(value)
        self._fold_v[0] = None

    @property
    def test_links(self):
        if self._test_links is None:
            self._test_links = TrackedLinks(self._fold.test_links_dict())
            self._fold_v[1] = self._test_links.version.n
        return self._test_links

    @test_links.setter
    def test_links(self, value):
        self._test_links = tracked(value)
        self._fold_v[1] = None

    @property
    def nlinks(self):
        if self._nlinks is None:
            self._nlinks = self._fold.nlinks_dict()
        return self._nlinks

    @nlinks.setter
    def nlinks(self, value):
        self._nlinks = value

    def links_changed(self):
        """Declare an edit the tables cannot see: a key added to or deleted from a dict that was
        assigned to `links` / `test_links` (row edits such as `d[k][1] += 1` are seen without
        it).  The tables re-read their source dicts and the device copy is rebuilt on the next
        call."""
        for t in (self._links, self._test_links):
            if isinstance(t, TrackedLinks):
                t.resync()
        self._links_version += 1

    # copy.deepcopy / pickle: the device engine is not copied (the copy builds its own on first
    # use, from freshly pulled host parameters) and the tables come back tracked
    def __getstate__(self):
        self._pull()
        state = dict(self.__dict__)
        state.update(_engine=None, _engine_key=None, _dev_fresh=False, _host_fresh=True)
        return state

    def __setstate__(self, state):
        self.__dict__.update(state)
        for name in ("_links", "_test_links"):
            t = self.__dict__.get(name)
            if t is not None and not isinstance(t, TrackedLinks):
                # (a new version: _fold_fresh then reads the copied table, not the parse)
                self.__dict__[name] = TrackedLinks(t)

    def _fold_fresh(self, which):
        """The parsed arrays still hold table `which` (nothing edited or replaced it)."""
        if self._fold is None or self._fold_v[which] is None:
            return False
        tab = self._links if which == 0 else self._test_links
        return tab is None or tab.version.n == self._fold_v[which]

    def _link_arrays(self, which):
        """(ids int32[E][3] in key order, counts int32[E][R]) of the train (0) / test (1) links."""
        if self._fold_fresh(which):
            f = self._fold
            return (f.train_ids, f.train_counts) if which == 0 else (f.test_ids, f.test_counts)
        return links_to_arrays(self.links if which == 0 else self.test_links, self.R)

    def _n_links(self, which=0):
        if self._fold_fresh(which):
            return int((self._fold.train_ids if which == 0 else self._fold.test_ids).shape[0])
        return len(self.links if which == 0 else self.test_links)

    def _ensure_engine(self):
        from .engine import EMEngine  # imports torch + the HIP library
        key = (self.K, self.P, self._links_version, version_of(self._links), version_of(self._test_links))
        if self._engine is None or self._engine_key != key:
            if self._engine is not None:
                self._pull()
                self._engine.close()
            eng = EMEngine(self.K, self.P, B=1, R=self.R, eps=self.eps, device=self._device)
            eng.set_links(_lib.SET_TRAIN, *self._link_arrays(0))
            eng.set_links(_lib.SET_TEST, *self._link_arrays(1))
            self._engine = eng
            self._engine_key = key
            self._dev_fresh = False
        return self._engine

    def _push(self):
        eng = self._ensure_engine()
        if not self._dev_fresh:
            self._pull()
            eng.upload(np.array(self._theta, dtype=np.float64)[None],
                       np.array(self._pr, dtype=np.float64)[None])
            self._dev_fresh = True
        return eng

    @property
    def engine(self):
        return self._push()

    # --------------------------------------------------- :106-170 (host RNG)
    def initialize_parameters(self, k_value=10):
        try:
            self.K = int(k_value)
        except ValueError:
            self.K = 10
        K, R, rnd = self.K, self.R, random.random
        self.vlikelihood = []
        self._theta = [[rnd() for _ in range(K)] for _ in range(self.P)]
        self.ntheta = [[0.0] * K for _ in range(self.P)]
        self._pr = [[[[rnd() for _ in range(R)] for _ in range(K)] for _ in range(K)] for _ in range(K)]
        self.npr = [[[[0.] * R for _ in range(K)] for _ in range(K)] for _ in range(K)]
        for g in range(self.P):
            total = 0.
            for v in self._theta[g]:
                total += v
            if total < self.eps:
                self._theta[g] = [rnd() for _ in range(K)]
            total = sum(self._theta[g])
            row = self._theta[g]
            for a in range(K):
                row[a] = row[a] / total if total != 0 else row[a] / (total + self.eps)
        for plane in self._pr:
            for line in plane:
                for cell in line:
                    total = 0.
                    for v in cell:
                        total += v
                    for r in range(R):
                        cell[r] = cell[r] / total if total != 0 else cell[r] / (total + self.eps)
        self._host_fresh = True
        self._dev_fresh = False

    # ------------------------------------------------- :218-318, :321-423
    def _register(self, names, gid):
        ids = []
        for g in names:
            if g not in self.gene_id:
                self.gene_id[g] = gid
                self.id_gene[gid] = g
                self.uniqueg[gid] = 0
                gid += 1
            n = self.gene_id[g]
            self.uniqueg[n] += 1
            ids.append(str(n))
        return ids, gid

    def _add(self, table, key, r):
        row = table.get(key)
        if row is None:
            table[key] = [0] * 2
            row = table[key]   # a tracked table stores its own row object
        row[r] += 1

    def get_input(self, argfilename, selectedinteractiontype="trigenic", cutoffvalue=-0.08, discard=0,
                  interactions='ALL'):
        try:
            gid = 0
            if selectedinteractiontype not in ('trigenic', 'digenic', '*'):
                raise ValueError("argument 2 selectedInteractionType must be trigenic, digenic or *")
            with codecs.open(argfilename, encoding='utf-8', mode='r') as fileref:
                first = fileref.readline()
                raw = len(re.split(r'\t+', first)) == 12
                for line in fileref.readlines():
                    fields = re.split(r'\t+', line)
                    if raw:
                        fields.pop(5)
                    if selectedinteractiontype != "*" and fields[4] != selectedinteractiontype:
                        continue
                    if interactions == 'ALL':
                        r = 1 if (float(fields[6]) < 0.05 and float(fields[5]) < cutoffvalue) else 0
                    else:
                        if float(fields[6]) >= 0.05:
                            continue
                        if float(fields[5]) < cutoffvalue:
                            r = 1
                        elif discard:
                            continue
                        else:
                            r = 0
                    names = fields[1].split('+') + [fields[3]]
                    ids, gid = self._register(names, gid)
                    names.sort()
                    ids.sort()
                    self._add(self.links, '_'.join(ids), r)
                    self._add(self.nlinks, '_'.join(names), r)
                self.P = len(self.id_gene)
        except ValueError as error:
            print(error)
        except IOError as error:
            print('Error, file does not exist or can\'t be read')
            print(error)
        self._links_version += 1

    def get_traintest(self, trainfile, testfile):
        # native reader (include/mmsbm_io.h) for the canonical format on a fresh Model; any other
        # input takes the reference-semantics loop below
        fold = None
        if NATIVE_INGEST and not self.gene_id and not self._n_links(0) and not self._n_links(1):
            from .ingest import parse_fold
            fold = parse_fold(trainfile, testfile)
        if fold is not None:
            self._fold = fold
            self.id_gene = dict(enumerate(fold.names))
            self.gene_id = {g: i for i, g in enumerate(fold.names)}
            self.uniqueg = dict(enumerate(fold.uniqueg.tolist()))
            self._links = self._nlinks = self._test_links = None
            self._fold_v = [0, 0]
            self.P = fold.P
            self._links_version += 1
            n_train = self._n_links(0)
            print('READ DATA train', n_train, n_train)
            print('READ DATA test', self._n_links(1))
            return
        try:
            gid = 0
            with codecs.open(trainfile, encoding='utf-8', mode='r') as fileref:
                for line in fileref.readlines():
                    fields = line.strip().split('\t')
                    names = fields[0].split('_')
                    r = int(fields[1])
                    ids, gid = self._register(names, gid)
                    names.sort()
                    ids.sort()
                    self._add(self.links, '_'.join(ids), r)
                    self._add(self.nlinks, '_'.join(names), r)
                self.P = len(self.id_gene)
            with codecs.open(testfile, encoding='utf-8', mode='r') as fileref:
                for line in fileref.readlines():
                    fields = re.split(r'\t+', line)
                    names = fields[0].split('_')
                    r = int(fields[1])
                    ids, gid = self._register(names, gid)
                    ids.sort()
                    self._add(self.test_links, '_'.join(ids), r)
                self.P = len(self.id_gene)
        except ValueError as error:
            print(error)
        except IOError as error:
            print('Error, file does not exist or can\'t be read')
            print(error)
            exit(1)
        self._links_version += 1
        print('READ DATA train', len(self.links), len(self.nlinks))
        print('READ DATA test', len(self.test_links))

    # ------------------------------------------------------------- :447-523
    def fold(self, fraction=0.2):
        test_set_size = int(len(self.links) * fraction)
        num_folds = int(1 / fraction)
        keys = list(self.links.keys())
        np.random.shuffle(keys)
        chunks = [keys[test_set_size * i: test_set_size * (i + 1)] for i in range(num_folds)]
        chunks[num_folds - 1] += keys[test_set_size * num_folds:]

        def line(triplet):
            rating = 0 if self.links[triplet][0] else 1
            names = sorted(self.id_gene[int(x)] for x in triplet.split("_"))
            return '_'.join(names) + '\t' + str(rating) + '\n'

        for f in range(num_folds):
            with codecs.open('test' + str(f) + '.dat', encoding='utf-8', mode="w+") as out:
                for t in chunks[f]:
                    out.write(line(t))
            with codecs.open('train' + str(f) + '.dat', encoding='utf-8', mode="w+") as out:
                for other in chunks[:f] + chunks[f + 1:]:
                    for t in other:
                        out.write(line(t))

    # ------------------------------------------------------ hot path (GPU)
    def make_iteration(self):
        """One EM iteration on the GPU (:984-1043).  ZeroDivisionError when a
        gene has no train link, like :1018."""
        eng = self._push()
        eng.iterate(1)
        self._host_fresh = False

    def make_iterations(self, n):
        """`n` back-to-back iterations without host round trips."""
        eng = self._push()
        eng.iterate(int(n))
        self._host_fresh = False

    def compute_likelihood(self, selected_set='train'):
        eng = self._push()
        which = _lib.SET_TRAIN if selected_set == 'train' else _lib.SET_TEST
        log_l = float(eng.loglik(which)[0])
        if selected_set == 'train':
            self.likelihood = log_l
        else:
            self.heldoutlikelihood = log_l
        return log_l

    # ------------------------------------------------------- :530-637
    def do_prediction(self, id1, id2, id3):
        try:
            ids = [int(id1), int(id2), int(id3)]
        except ValueError:
            ids = [self.gene_id[id1], self.gene_id[id2], self.gene_id[id3]]
        # the reference indexes the theta list (:537): an id >= P raises IndexError and a
        # negative id counts from the end; the device kernel is only ever handed ids in [0, P)
        for n, g in enumerate(ids):
            if not -self.P <= g < self.P:
                raise IndexError("list index out of range")
            ids[n] = g % self.P
        eng = self._push()
        return float(eng.predict(np.array([ids], dtype=np.int32))[0, 0])

    def predict_novel(self, n, exclude=("train", "test"), mask=None):
        """The n most probable triples of distinct genes outside the `exclude`d link tables, best
        first: [probability, "i_j_k", [name1, name2, name3]] with the key as `links` spells it
        (:349-358), the probability of do_prediction (:530-547) and the names sorted as the
        `nlinks` keys are.  One scan of all C(P, 3) triples on the GPU (engine.scan_top).  mask: a
        pair mask (Model.pair_mask): no triple that contains a blocked pair of genes is listed."""
        from .scan import known_keys
        eng = self._push()
        scores, ids = eng.scan_top(int(n), known_keys(self, exclude), sample=0, **_masked(mask))
        return self._rows(scores, ids)

    def predict_novel_any(self, n, exclude=("train", "test"), mask=None):
        """predict_novel for any n >= 1: above the scan's cap of 4096 rows, censuses bracket the
        score of rank n and one threshold scan fetches what lies at or above it
        (engine.scan_top_any).  Up to the cap it is predict_novel.  mask: a pair mask
        (Model.pair_mask): no triple that contains a blocked pair of genes is listed; the route is
        the same, through the masked calls."""
        from .scan import known_keys
        scores, ids = self._push().scan_top_any(int(n), known_keys(self, exclude), sample=0, **_masked(mask))
        return self._rows(scores, ids)

    def pair_mask(self, genes=None, pairs=None):
        """The pair mask of the `mask=` keywords (scan.pair_mask): genes = the allowed genes (every
        pair that touches another gene is blocked), pairs = pairs of genes to block; ids or names as
        do_prediction takes them (KeyError on an unknown name, IndexError on an id outside the
        table).  Both None: the mask that blocks nothing."""
        from .scan import pair_mask, resolve_genes
        if genes is not None:
            genes = resolve_genes(self, list(genes))
        if pairs is not None:
            pairs = np.asarray(resolve_genes(self, [g for pair in pairs for g in pair]), dtype=np.int64).reshape(-1, 2)
        return pair_mask(self.P, pairs=pairs, genes=genes)

    def predict_network(self, threshold=0.5, exclude=("train", "test"), limit=1 << 26, mask=None):
        """Every triple of distinct genes outside the `exclude`d link tables with
        P(r = 1) >= threshold, best first, equal probabilities by key: the predicted trigenic
        network at that cut, in predict_novel's row format.  novel_census([threshold]) is its
        length; more than `limit` rows raise ValueError (scan.LimitError) before the list is
        formed.  One census and one threshold scan of all C(P, 3) triples on the GPU
        (engine.scan_above).  mask: as for predict_novel_any."""
        from .scan import known_keys
        scores, ids = self._push().scan_above(float(threshold), known_keys(self, exclude), sample=0,
                                              limit=limit, **_masked(mask))
        return self._rows(scores, ids)

    def _gene_arg(self, gene):
        """A gene id or name as do_prediction takes them -> id in [0, P) (IndexError like :537)."""
        try:
            g = int(gene)
        except ValueError:
            g = self.gene_id[gene]
        if not -self.P <= g < self.P:
            raise IndexError("list index out of range")
        return g % self.P

    def _rows(self, scores, ids):
        return [[float(p), "_".join(str(int(g)) for g in row), sorted(self.id_gene[int(g)] for g in row)]
                for p, row in zip(scores, ids)]

    def predict_partners(self, gene, n, exclude=("train", "test"), mask=None):
        """The n most probable triples that contain `gene` (an id or a name) and two other, distinct
        genes, outside the `exclude`d link tables, best first; rows shaped like predict_novel's:
        [probability, "i_j_k", [name1, name2, name3]], the gene included in the key.  One partner
        scan of its (P - 1)(P - 2) / 2 pairs on the GPU (engine.partners_top).  mask: a pair mask
        (Model.pair_mask): no triple that contains a blocked pair of genes is listed, the pairs with
        `gene` included."""
        from .scan import partner_known
        g = self._gene_arg(gene)
        eng = self._push()
        (scores, ids), = eng.partners_top([g], int(n), partner_known(self, [g], exclude), sample=0, **_masked(mask))
        return self._rows(scores, ids)

    def predict_third(self, gene1, gene2, n, exclude=("train", "test"), mask=None):
        """The n most probable third genes of the pair (gene1, gene2), best first, rows as
        predict_partners gives them.  The P - 2 listed triples go through the predict kernel and a
        host sort under the scan's order (probability descending, equal ones by packed key).  mask:
        a pair mask (Model.pair_mask), applied on the host: a triple that contains a blocked pair is
        left out, so a blocked query pair gives []."""
        from .scan import check_pair_mask, pack_keys, parse_exclude, rank_of, rank_order
        g1, g2 = self._gene_arg(gene1), self._gene_arg(gene2)
        if g1 == g2:
            raise ValueError("predict_third needs two different genes")
        order = rank_order(self.P)
        rank = rank_of(order)
        third = np.array([g for g in range(self.P) if g != g1 and g != g2], dtype=np.int64)
        pos = np.sort(np.stack([np.full(third.size, rank[g1]), np.full(third.size, rank[g2]), rank[third]],
                               axis=1), axis=1)
        ids = order[pos].astype(np.int32)                      # key order: slots 1, 2, 3
        tables = [self.links if name == "train" else self.test_links for name in parse_exclude(exclude)]
        keep = np.array([not any("_".join(str(int(g)) for g in row) in t for t in tables) for row in ids],
                        dtype=bool)
        if mask is not None:
            mask = check_pair_mask(mask, self.P)
            a, b, c = pos[:, 0], pos[:, 1], pos[:, 2]      # sorted positions: the mask is read at x < y
            bit = lambda x, y: ((mask[x, y >> 5] >> (y & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)  # noqa: E731
            keep &= ~(bit(a, b) | bit(a, c) | bit(b, c))
        ids = ids[keep]
        if not ids.shape[0]:
            return []
        scores = self._push().predict(ids)[0]
        top = np.lexsort((pack_keys(ids, rank, self.P), -scores))[:int(n)]
        return self._rows(scores[top], ids[top])

    def _pair_args(self, pairs):
        return np.array([[self._gene_arg(g) for g in pair] for pair in pairs], dtype=np.int64).reshape(-1, 2)

    def predict_screen(self, pairs, n, exclude=("train", "test"), mask=None):
        """For each query pair of genes (ids or names), its n most probable third genes outside the
        `exclude`d link tables, best first: one list per pair of rows [probability, "i_j_k",
        [name1, name2, name3]] as predict_partners gives them.  Every pair of the call goes through
        one screen scan on the GPU (engine.screen_top).  mask: a pair mask (Model.pair_mask): a third
        gene that forms a blocked pair with either gene of the query is left out.  ValueError on a
        pair of one gene."""
        from .scan import screen_known
        pairs = self._pair_args(pairs)
        lists = self._push().screen_top(pairs, int(n), screen_known(self, pairs, exclude), sample=0, mask=mask)
        return [self._rows(scores, ids) for scores, ids in lists]

    def predict_profiles(self, pairs, exclude=("train", "test"), mask=None):
        """-> ndarray f64 [Q][P]: row i = the probability of the triple of pairs[i] (ids or names)
        with every gene id, the pair's predicted interaction profile across the array; NaN at the
        pair's own genes, at the third genes the `exclude`d tables hold for it and at what `mask`
        blocks (engine.screen_scores)."""
        from .scan import screen_known
        pairs = self._pair_args(pairs)
        return self._push().screen_scores(pairs, screen_known(self, pairs, exclude), sample=0, mask=mask)

    # ---------------------------------------------------------- score census
    # Exactness: the counts are exact for the scan's score bits; a listed triple's probability comes
    # from the predict kernel, which sums in another order, so a triple within rounding distance
    # (about 1e-12 relative) of another triple's score may be placed on either side of it.
    def novel_census(self, thresholds, exclude=("train", "test"), mask=None):
        """-> (counts int64[len(thresholds)], total): counts[i] = the triples of distinct genes
        outside the `exclude`d link tables with P(r = 1) >= thresholds[i], total = all of them.
        Stands to engine.census as predict_novel stands to scan_top: one pass over all C(P, 3)
        triples on the GPU per 1024 thresholds.  mask: as for predict_novel_any."""
        from .scan import known_keys
        return self._push().census(thresholds, known_keys(self, exclude), sample=0, **_masked(mask))

    def _ranked(self, ids, exclude):
        from .scan import known_keys, ranks_of
        return ranks_of(self._push(), ids, known_keys(self, exclude), sample=0)

    def novel_rank(self, triples, exclude=("train", "test")):
        """Where listed triples stand genome-wide: one row [rank, probability, "i_j_k"] per triple
        (three gene ids or names each, as do_prediction takes them).  probability is
        do_prediction's of the triple in key order, rank 1 + the number of triples of distinct genes outside the `exclude`d
        tables that score strictly above it (a listed triple that is itself excluded gets the rank
        it would have had), the key as `links` spells it (:349-358)."""
        from .scan import rank_of, rank_order
        order = rank_order(self.P)
        rank = rank_of(order)
        genes = np.array([[self._gene_arg(g) for g in t] for t in triples], dtype=np.int64).reshape(-1, 3)
        ids = order[np.sort(rank[genes], axis=1)].astype(np.int32).reshape(-1, 3)   # key order
        probs, ranks = self._ranked(ids, exclude)
        return [[int(r), float(p), "_".join(str(int(g)) for g in row)] for r, p, row in zip(ranks, probs, ids)]

    def heldout_ranks(self):
        """The genome-wide rank of every test link among everything not trained on: one row
        [rank, probability, key, real] per test link (real as in `results`), ordered by rank, equal
        ranks by key.  Only the train links are excluded."""
        from .scan import heldout_rows
        ids, counts = self._link_arrays(1)
        if not ids.shape[0]:
            return []
        probs, ranks = self._ranked(ids, ("train",))
        return heldout_rows(ids, counts, probs, ranks)

    # ----------------------------------------------------------- pair census
    # The question of a trigenic screen: its unit of work is a double-mutant query (a pair of genes
    # crossed against the whole array), so the pair to build next is the one with the most
    # predicted, unmeasured interactions.
    def novel_pair_counts(self, thresholds, exclude=("train", "test"), mask=None):
        """-> int32 [P][P][len(thresholds)] in gene ids: [i][j][m] = the triples of distinct genes
        outside the `exclude`d link tables that contain genes i and j with P(r = 1) >= thresholds[m].
        Symmetric, zero diagonal.  One pass over all C(P, 3) triples on the GPU per 8 thresholds
        (engine.pair_census).  mask: as for predict_novel_any; a blocked pair's counts are zero."""
        from .scan import known_keys
        return self._push().pair_census(thresholds, known_keys(self, exclude), sample=0, **_masked(mask))

    def predict_query_pairs(self, n, threshold=0.5, exclude=("train", "test"), mask=None):
        """The n pairs of genes with the most such triples at or above `threshold`, best first
        (equal counts by the pair's key): rows [count, eligible, "i_j", [name1, name2]] with the
        key as `links` spells keys (:349-358), the names sorted as in predict_novel, and eligible =
        the pair's triples outside the `exclude`d tables in all (engine.pairs_top).  mask: as for
        predict_novel_any: count and eligible then leave out the triples with a blocked pair, so with
        the genes of a strain array allowed (Model.pair_mask(genes=...)) the ranking is that of the
        double-mutant queries over the triples the array can build."""
        from .scan import known_keys, pair_rows
        counts, eligible, ids = self._push().pairs_top(int(n), float(threshold), known_keys(self, exclude),
                                                       sample=0, **_masked(mask))
        return pair_rows(self.id_gene, counts, eligible, ids)

    def novel_gene_counts(self, thresholds, exclude=("train", "test"), mask=None):
        """-> int64 [P][len(thresholds)]: per gene id, the triples of distinct genes outside the
        `exclude`d link tables that contain it with P(r = 1) >= each threshold (engine.gene_census).
        mask: as for predict_novel_any."""
        from .scan import known_keys
        return self._push().gene_census(thresholds, known_keys(self, exclude), sample=0, **_masked(mask))

    def calculate_test_set_results(self):
        tids, _ = self._link_arrays(1)
        keys = list(self.test_links.keys())
        probs = self._push().predict(tids)[0] if keys else []
        self.results = []
        for p, key in zip(probs, keys):
            self.results.append([float(p), key, 0 if self.test_links[key][0] else 1])
        self.results.sort()
        self.results.reverse()

    def calculate_metrics(self):
        if self._fold_fresh(0):
            positives = int((self._fold.train_counts[:, 1] == 1).sum())
        else:
            positives = sum(1 for n in self.links.values() if n[1] == 1)
        positives_fraction = positives / self._n_links(0)
        positives_number = int(positives_fraction * self._n_links(1))
        cut_value = 0
        if positives_number < len(self.results):
            cut_value = self.results[positives_number][0]
        pos = np.array([row[0] for row in self.results if row[2]], dtype=np.float64)
        neg = np.sort(np.array([row[0] for row in self.results if not row[2]], dtype=np.float64))
        # pairs with positive strictly above negative (:611-615), by rank instead of O(n+ n-)
        better = int(np.searchsorted(neg, pos, side='left').sum())
        auc = better / (len(pos) * len(neg))
        tp = fp = fn = tn = 0
        for row in self.results:
            if row[0] >= cut_value:
                if row[2]:
                    tp += 1
                else:
                    fp += 1
            elif row[2]:
                fn += 1
            else:
                tn += 1
        return [tp / (tp + fp), tp / (tp + fn), fp / (fp + tn), auc]

    # ------------------------------------------------------- :793-904
    def to_string(self):
        def print_tuples(tuples):
            txt = '\nPredicted Interaction\tID of genes\tReal Interaction\n'
            for row in tuples:
                txt += str(row[0]) + '\t' + str(row[1]) + '\t' + str(row[2]) + '\n'
            return txt

        text = "Max Likelihood:\t" + str(self.likelihood) + "\n"
        text += "Held-out Likelihood:\t" + str(self.compute_likelihood('test')) + "\n"
        text += "Number of genes (P):\t" + str(self.P) + "\n"
        text += "Number of links:\t" + str(self._n_links(0)) + "\n"
        text += "Number of groups of genes (K):\n" + str(self.K) + "\n"
        text += "Number of possible ratings (R):\n" + str(self.R) + "\n\n"
        self.calculate_test_set_results()
        metrics = self.calculate_metrics()
        text += "\nMetrics:\nPrecision\tRecall\tFallout\tAUC\n"
        text += str(metrics[0]) + "\t" + str(metrics[1]) + "\t" + str(metrics[2]) + "\t" + str(metrics[3])
        text += "\nTest set:" + str(print_tuples(self.results))
        return text

    def to_file(self, name_file=None):
        try:
            if name_file is None:
                name_file = "out.txt"
            # the file is created before the text is built (:898-899): if to_string raises, an
            # empty file stays behind, which the CLI's resume rule (:1256) then skips
            with codecs.open(name_file, encoding='utf-8', mode="w+") as fileref:
                fileref.write(self.to_string())
        except IOError:
            print("I/O error")

    # ------------------------------------------------------- :915-1067
    def compare_links(self, arg_model):
        return [link for link in self.nlinks.keys() if link not in arg_model.nlinks]

    def compare_genes(self, arg_model):
        return [gene for gene in self.gene_id.keys() if gene not in arg_model.gene_id]

    def compare_dataset(self, arg_model):
        if not self.compare_links(arg_model):
            print("First dataset is subgraph of second dataset for links")
            node = 1
        else:
            print("First dataset is not subgraph of second dataset for links")
            node = 0
        if not self.compare_genes(arg_model):
            print("First dataset is subgraph of second dataset for nodes")
            link = 1
        else:
            print("First dataset is not subgraph of second dataset for nodes")
            link = 0
        return link and node
