"""What the GPU tests of the scan families share: the engine of a parameter set, the cached cases
with their numpy reference (tests/scan_ref.py) and the families' C calls as C sees them.  Nothing
here imports the engine or torch before a test asks for them."""
import collections
import ctypes
import functools

import numpy as np

import scan_ref
from golden_util import load


def engine(thetas, prs):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    thetas, prs = np.asarray(thetas), np.asarray(prs)
    B, P, K = thetas.shape
    eng = EMEngine(K, P, B=B)
    eng.upload(thetas, prs)
    return eng


def reference(theta, pr):
    """scan_ref.ref_scores, read-only: (scores, packed keys ascending)."""
    scores, keys = scan_ref.ref_scores(theta, pr)
    assert (np.diff(keys) > 0).all()
    for a in (scores, keys):
        a.setflags(write=False)
    return scores, keys


@functools.lru_cache(maxsize=None)
def random_case(K, P, seed):
    """(theta [P][K], pr, reference scores, reference keys) of one random sample; computed once."""
    th, pr = scan_ref.random_params(K, P, seed)
    return (th[0], pr[0]) + reference(th[0], pr[0])


Fixture = collections.namedtuple("Fixture", "theta pr P model known scores keys")
EXCLUDES = ((), ("train",), ("train", "test"))


@functools.lru_cache(maxsize=None)
def fixture_case(fold, name, it):
    """One committed fixture at iteration `it`: theta, pr, P, the model of its fold, the known keys
    of each exclude set {exclude: keys} and the reference scores and keys; computed once."""
    from trigenicinteractionpredictor_amd import Model
    from trigenicinteractionpredictor_amd.scan import known_keys
    _, vec, train, test = load(fold, name)
    theta, pr = vec["theta_%d" % it], vec["pr_%d" % it]
    m = Model()
    m.get_traintest(train, test)
    assert m.P == theta.shape[0]
    return Fixture(theta, pr, m.P, m, {ex: known_keys(m, ex) for ex in EXCLUDES}, *reference(theta, pr))


SENTINEL = -7


class Raw:
    """One family's C entry as C sees it, on the engine's own rank order and scratch
    (EMEngine.scan_order, scan_workspace(family, *size_args)).  call() launches on outputs the
    caller made, usually full() of a sentinel, synchronises and returns the code; intact() says
    whether every output word still holds SENTINEL."""
    ENTRY = {"scan": "mmsbm_scan_topn", "partners": "mmsbm_partners_topn", "census": "mmsbm_scan_census",
             "pair_census": "mmsbm_pair_census", "scan_above": "mmsbm_scan_above"}

    def __init__(self, eng, family, *size_args):
        import torch
        self.eng, self.family, self.torch = eng, family, torch
        self.ws = eng.scan_workspace(family, *size_args)
        assert self.ws.numel() > 0

    def full(self, shape, dtype, value=SENTINEL):
        return self.torch.full(shape, value, dtype=dtype, device=self.eng.device)

    def upload(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.eng.device)

    def call(self, mid, outs, sample=0, known=None, n_known=None, queries=None, ws=None, replace=()):
        """mid: the entry's arguments between the sample and the workspace; outs: its output
        tensors, None for NULL; known: a key table to upload (n_known overrides its length);
        queries: the partner scan's int32 gene ids, in place of the key table; ws: (pointer, bytes)
        in place of the scratch; replace: (index, value) pairs put into the argument list last."""
        eng = self.eng
        known_d = None if known is None else self.upload(known)
        keys = [None if known is None else known_d.data_ptr(), 0 if known is None else int(known.size)]
        if n_known is not None:
            keys[1] = n_known
        if queries is not None:
            keys = [queries.ctypes.data_as(ctypes.c_void_p), int(queries.size), None, None]
        self.outs = outs
        args = [eng.ctx, eng.scan_order.data_ptr(), *keys, eng.theta.data_ptr(), eng.pr.data_ptr(), sample, *mid,
                *((self.ws.data_ptr(), self.ws.numel()) if ws is None else ws),
                *[None if o is None else o.data_ptr() for o in outs], eng._stream()]
        for i, value in replace:
            args[i] = value
        rc = getattr(eng.lib, self.ENTRY[self.family])(*args)
        self.torch.cuda.synchronize(eng.device)
        return rc

    def intact(self):
        return all(bool((o == SENTINEL).all()) for o in self.outs)


# ------------------------------------------------------------------ the planted model's scale cases
def planted_engine(model, mode="prefix"):
    """The engine of a planted model (tests/planted_ref.py).  mode "single": a B = 1 engine on
    slot 0; "prefix": all its slots with an active prefix of planted_ref.SCALE_ACTIVE."""
    import planted_ref
    if mode == "single":
        return engine(model.theta[:1], model.pr[:1])
    eng = engine(model.theta, model.pr)
    eng.set_active(planted_ref.SCALE_ACTIVE)
    return eng


def known_of(model, with_known, stats=None):
    """The scale cases' known keys (planted_ref.scale_known; the 50 best elites under `stats`,
    default the ensemble mean and slot 0, among them), or None."""
    import planted_ref as pl
    if not with_known:
        return None
    return pl.scale_known(model, [pl.stat(model, ns=pl.SCALE_ACTIVE), pl.stat(model, sample=0)]
                          if stats is None else stats)


def check_list(got, want, P, atol=None):
    """A top-N list (scores, ids) against the reference's (scores, packed keys): ids exactly and in
    order; scores at scan_ref.RTOL (a spread: the absolute bound `atol`)."""
    (s, ids), (want_s, want_k) = got, want
    assert s.dtype == np.float64 and ids.dtype == np.int32 and ids.shape == (want_k.size, 3)
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
    if atol is None:
        np.testing.assert_allclose(s, want_s, rtol=scan_ref.RTOL, atol=0)
    else:
        np.testing.assert_allclose(s, want_s, rtol=0, atol=atol)
