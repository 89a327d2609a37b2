"""Catalogue top-K recommendation: which K items does a trained model recommend to user u?

The reference has no such call (its ranking metric scores one positive against five sampled negatives,
eval.py:64-92).  Three of its models score a pair as

    score(u, i) = <user vector, item vector> + user scalar + item scalar

so a whole catalogue is ranked by one fused kernel (r4r_topk_dot, csrc/topk.hip) over cached per-item vectors,
with no forward per pair:

    bias_only (MF.py:48-49)   vectors of width 0
    MF_dot    (MF.py:56-58)   the embedding tables in place
    deepconn  (DeepCoNN.py:57-66)   the FM over [user tower | item tower] separates (``fold_fm``): one tower
                              forward per ITEM (cached by ``Catalogue.refresh``), one per requested user, and a
                              rank-8 dot per pair.

Every other model type has a ReLU layer or an FM over a per-pair transform between the two sides and is refused
by ``Catalogue`` with the reason (``catalogue_limits``).  Two of them are served by ``ReluCatalogue``: the first
Linear of a Linear -> ReLU head over [user | item] separates, W [x_u ; x_i] + b = (W_u x_u + b) + W_i x_i, and
everything after the ReLU is linear down to one scalar, so

    score(u, i) = sum_j w_j relu(qa[u][j] + ca[i][j]) + <qp[u], cp[i]> + user scalar + item scalar

    deepconn++ (DeepCoNN.py:68-72)                     one tower forward per item (cached), one per requested user
    NeuMF      (NeuMF.py:25-38 / 60-74 / 120-143)      stages GMF, MLP and NeuMF: the embedding tables through one
                                                       small matmul

ranked by r4r_topk_relu / r4r_rank_relu (csrc/topk_relu.hip; ``fold_relu_head`` has the table, ``relu_catalogue_limits``
the limits).  ``main``'s hooks (``recommend_k``, ``catalogue_metrics_k``) build whichever class serves the model
through ``make_catalogue``; they accept deepconn++ and still refuse NeuMF, which is served through the class and
``eval.eval_catalogue(catalogue=ReluCatalogue(...))`` only.

NARRE's head is Linear -> ReLU -> Linear over the ELEMENTWISE PRODUCT of the two sides, and each side's attention reads
only that side's own neighbours (NARRE.py:110-113; nothing is removed for a rating outside the training split,
data.py:240-246), so per-user and per-item vectors exist and

    score(u, i) = sum_j w_j relu(<W_j, au[u] * ai[i]> + b_j) + user scalar + item scalar

is ranked by r4r_topk_hmlp / r4r_rank_hmlp (csrc/topk_hmlp.hip: an MFMA scan whose A operand is W) through
``NarreCatalogue`` (``narre_catalogue_limits`` has the limits) and ``eval.eval_catalogue(catalogue=NarreCatalogue(...))``;
``main``'s hooks still refuse it.

The TransNets score a pair at test time with source_fm over Linear -> ReLU -> Linear of [user tower | item tower]
(TransNet.py:105-119; eval.py:31-32 takes output[0]); both towers read one side's document only.  The first Linear
separates as deepconn++'s does, and an FM of a linear image of h = relu(.) is a short sum of signed squares and one linear
term of y = W h + b (``fold_transnet_head``), so

    score(u, i) = sum_j y_j (s_j y_j + l_j) + user scalar + item scalar,    y = W [relu(qa[u] + ca[i]) ; qp[u] + cp[i]] + b

is ranked by r4r_topk_rfm / r4r_rank_rfm (csrc/topk_rfm.hip: the same scan with relu(q + c) as the B operand and squares
in the epilogue) through ``TransNetCatalogue`` (``transnet_catalogue_limits`` has the limits) and
``eval.eval_catalogue(catalogue=TransNetCatalogue(...))``; ``main``'s hooks still refuse them.

MF (MF.py:45-49) scores a pair with an FM over [Linear -> ReLU -> Linear of [user | item] | user * item].  The first
Linear separates again, the FM's squares are signed squares of y = W [h ; m] + b with h = relu(.) and m = user * item, and
what is left is per column of x = [h ; m] -- the square of a product column is that column's own x^2
(``fold_mf_head``) -- so

    score(u, i) = sum_j s_j y_j^2 + sum_m x_m (g_m x_m + e_m) + user scalar + item scalar,
    y = W x + b,   x = [relu(qa[u] + ca[i]) ; ue[u] * ie[i]]

is ranked by r4r_topk_pfm / r4r_rank_pfm (csrc/topk_pfm.hip: the scan with product columns, a column sum carried by the
lanes that form x, and the 2 L x 2 L head resident in LDS) through ``MFCatalogue`` (``mf_catalogue_limits`` has the limits)
and ``eval.eval_catalogue(catalogue=MFCatalogue(...))``.  ``main``'s hooks still refuse MF, ``catalogue_limits`` and
``_REFUSED`` still give the reason ``Catalogue`` cannot rank it, and ``transnet_catalogue_limits`` still says that no class
serves it: those texts are pinned by tests and predate ``MFCatalogue``.

Where the towers of the text families run from is ``Catalogue``'s ``towers``: 'host' builds every owner's document with
numpy and calls the tower once per ``tower_batch`` owners; 'device' builds them from the HBM-resident pools and enqueues
the same per-chunk launches from C (r4r_tower_span_fwd, csrc/tower_span.hip) -- the same bits, one call per pass.

Slates -- a candidate list per user -- are ranked by every class: ``recommend_among`` gives the k best of each user's
own list (re-ranking what a retrieval stage, a filter or a basket hands over) and ``rank_among`` the place of an item
among given candidates, the sampled-negative protocol of eval.py:64-92 at any number of negatives and any K
(``sample_negatives`` draws them, ``eval.eval_sampled`` reports the metrics, ``slates_csr`` checks a list).  Both go
through r4r_slate_topk_<form> / r4r_slate_rank_<form> (csrc/slate_device.h): scalar chains over the cached two sides, in
``score_pairs``' bits and the same order, without a scan of the catalogue.

NARRE's review-level explanations -- which reviews of an item, which of a user's own, carry its attended vector -- are
``NarreCatalogue.explain``: the k heaviest real reviews per owner by the model's attention weights, from
r4r_narre_explain (csrc/narre_explain.hip), the eval-mode attention for R, L up to 64 that keeps its weights.

Phrase explanations -- which three-word windows of an owner's reviews carry its latent vector -- are ``explain_words`` on
every text class: the windows that won the max-pool of the side's TextCNN tower (common_pytorch_models.py:29-31), listed
by r4r_textcnn_phrases (csrc/phrases.hip) from the pooled values and argmax positions the tower forward returns, per chunk
from the host or inside one r4r_tower_span_phrases call; NARRE gets one list per review, e.g. of the reviews ``explain`` names.

Pair explanations -- why THIS item for THIS user -- are ``pair_weights`` / ``explain_pair`` on ``Catalogue`` (deepconn),
``ReluCatalogue`` (deepconn++) and ``TransNetCatalogue``: the gradient of one pair's predicted rating with respect to each
tower's pooled features, from r4r_pair_grad (csrc/pair_grad.hip) over the model's raw head parameters, handed to
``explain_words`` as its per-row weights.  NARRE is refused (its gradient runs through the attention's softmax).

There is no torch fallback: the order (score descending, ties by ascending item id, include/r4r.h) has one
definition, the kernels'.
"""
from collections import namedtuple

import numpy as np
import torch

from . import _lib, ops
from ._lib import ptr
from .data import NEIGHBOURS

SUPPORTED = ('bias_only', 'MF_dot', 'deepconn')
TOWERS = ('host', 'device')         # where a text catalogue builds its documents and enqueues its tower forwards from
MAX_D, MAX_K, FM_RANK = 256, 128, 8

_REFUSED = {
    'deepconn++': 'its head is Linear -> ReLU over [user | item] (DeepCoNN.py:68-72): the pair score is not bilinear',
    'NARRE': 'its head is Linear -> ReLU over the elementwise product of the two sides (NARRE.py:38-43,121-123): the pair score is not bilinear',
    'transnet': 'its score is an FM over a ReLU transform of the pair\'s joint document (TransNet.py): not bilinear',
    'transnet++': 'its score is an FM over a ReLU transform of the pair\'s joint document (TransNet.py): not bilinear',
    'MF': 'its head is Linear -> ReLU over [user | item] before the FM (MF.py:60-66): the pair score is not bilinear',
    'NeuMF': 'its MLP branch is Linear -> ReLU over [user | item] (NeuMF.py): the pair score is not bilinear',
}


def _latent_size(hyper_params):
    return int(hyper_params.get('latent_size', 10))        # (the default of main.native_step_limits)


# Who serves which model types, in the order the classes came: each later ``*_catalogue_limits`` refuses the types of
# the classes before its own with these words.
_SERVED = (
    (SUPPORTED, 'is a dot product plus two scalars: Catalogue serves it'),
    (('deepconn++', 'NeuMF'), 'has a ReLU-sum head: ReluCatalogue serves it'),
    (('NARRE',), 'has a product-MLP head: NarreCatalogue serves it'),
    (('transnet', 'transnet++'), 'has a ReLU-FM head: TransNetCatalogue serves it'),
)


def _served_before(mt, n):
    """The refusal of a model type that one of the first ``n`` classes serves, else None."""
    for types, what in _SERVED[:n]:
        if mt in types:
            return 'model_type %r %s' % (mt, what)
    return None


def catalogue_limits(hyper_params):
    """None when ``Catalogue`` can rank this configuration, else the reason it cannot."""
    mt = hyper_params['model_type']
    if mt in _REFUSED:
        return 'model_type %r has no catalogue form: %s' % (mt, _REFUSED[mt])
    if mt not in SUPPORTED:
        return 'model_type %r has no catalogue form' % (mt,)
    if mt == 'MF_dot' and _latent_size(hyper_params) > MAX_D:
        return 'latent_size %d > %d' % (_latent_size(hyper_params), MAX_D)
    return None


def fold_fm(V, lin_w, lin_b, global_bias, latent, side, dtype=torch.float32):
    """One side of DeepCoNN's FM head (common_pytorch_models.py:49-57) over cat = [a | c] as (vec [n, 8], bias [n]):

        fm(cat) + g = sum_f p_f q_f + [1/2 (sum_f p_f^2 - a^2 . Vu^2) + wu . a + lin.bias + g]      (user)
                                    + [1/2 (sum_f q_f^2 - c^2 . Vi^2) + wi . c]                     (item)

    with V = [Vu ; Vi], lin.weight = [wu | wi], p = a Vu, q = c Vi.  ``latent`` [n, L] is a (side 'user') or c
    ('item').  Plain torch on whatever device the inputs live on, computed in float64 and rounded once to ``dtype``:
    it runs once per refresh, and its own rounding stays out of the score."""
    if side not in ('user', 'item'):
        raise ValueError("fold_fm: side must be 'user' or 'item', got %r" % (side,))
    x = latent.detach().to(torch.float64)
    L = x.shape[1]
    V64, w64 = V.detach().to(torch.float64), lin_w.detach().to(torch.float64).reshape(-1)
    if V64.shape[0] != 2 * L or w64.numel() != 2 * L:
        raise ValueError('fold_fm: V %s / lin.weight %s do not match latent width %d' % (tuple(V.shape), tuple(lin_w.shape), L))
    rows = slice(0, L) if side == 'user' else slice(L, 2 * L)
    Vs, ws = V64[rows], w64[rows]
    vec = x @ Vs
    bias = 0.5 * ((vec * vec).sum(1) - ((x * x) @ (Vs * Vs)).sum(1)) + x @ ws
    if side == 'user':
        bias = bias + lin_b.detach().to(torch.float64).reshape(()) + global_bias.detach().to(torch.float64).reshape(())
    return vec.to(dtype), bias.to(dtype)


def eligible_items(hyper_params, train_reader, candidates=None):
    """Sorted int64 ids a list may contain: ``candidates``, or every item with a training rating (the keys of
    ``train_reader.item_count``).  The padding rows total_items and total_items + 1 are never eligible."""
    n_items = int(hyper_params['total_items'])
    if candidates is None:
        ids = np.fromiter((int(i) for i in train_reader.item_count), dtype=np.int64, count=len(train_reader.item_count))
    else:
        ids = np.asarray(candidates, dtype=np.int64).reshape(-1)
    ids = np.unique(ids)
    if len(ids) and (ids[0] < 0 or ids[-1] >= n_items):
        raise ValueError('catalogue: candidate ids must lie in [0, total_items = %d)' % n_items)
    return ids


def seen_csr(train_reader, n_users):
    """(off int64 [n_users + 1], ids int64): per user the distinct items of its training ratings, ascending."""
    data = train_reader.data
    if len(data) == 0:
        return np.zeros(n_users + 1, np.int64), np.zeros(0, np.int64)
    u, i = data[:, 0].astype(np.int64), data[:, 1].astype(np.int64)
    if u.min() < 0 or u.max() >= n_users:
        raise ValueError('catalogue: training user id outside [0, %d)' % n_users)
    pairs = np.unique(np.stack([u, i], 1), axis=0)             # sorted by user, then item; distinct
    off = np.zeros(n_users + 1, np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=n_users), out=off[1:])
    return off, np.ascontiguousarray(pairs[:, 1])


def _host_ints(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    a = np.asarray(a)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise ValueError('slates: integer ids expected, got %s' % a.dtype)
    return a.astype(np.int64)


def _csr_rows(off):
    """The row of every entry of a CSR."""
    return np.repeat(np.arange(len(off) - 1, dtype=np.int64), np.diff(off))


def slates_csr(slates, n, n_c):
    """Per-query candidate lists ("slates", include/r4r.h) as what r4r_slate_*_<form> take
    -> (off int64 [n + 1], ids int64, longest): host arrays and the length of the longest slate.

    ``slates``: a 2-D integer array or tensor [n, C] whose negative entries are padding, or a TUPLE (off, ids).  The
    entries keep their order.  ValueError for another row count than ``n``, an id outside [0, n_c) and an id repeated
    within one slate (the kernels count on distinct ids).  Vectorised: no Python loop per row."""
    n = int(n)
    if isinstance(slates, tuple):
        if len(slates) != 2:
            raise ValueError('slates: a tuple is (off, ids), got %d members' % len(slates))
        off, ids = _host_ints(slates[0]).reshape(-1), _host_ints(slates[1]).reshape(-1)
        if len(off) != n + 1:
            raise ValueError('slates: off has %d entries for %d rows (n + 1 expected)' % (len(off), n))
        if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != len(ids):
            raise ValueError('slates: off must ascend from 0 to len(ids) = %d' % len(ids))
        if len(ids) and ids.min() < 0:
            raise ValueError('slates: id %d outside [0, %d)' % (ids.min(), n_c))
    else:
        a = _host_ints(slates)
        if a.ndim != 2:
            if a.size or n:
                raise ValueError('slates: a 2-D array [n, C] or a tuple (off, ids) expected, got shape %r' % (a.shape,))
            a = a.reshape(0, 0)                                # (an empty list of rows)
        if a.shape[0] != n:
            raise ValueError('slates: %d rows for %d queries' % (a.shape[0], n))
        keep = a >= 0
        off = np.zeros(n + 1, np.int64)
        np.cumsum(keep.sum(1), out=off[1:])
        ids = a[keep]                                          # (row-major: each slate in its own order)
    if len(ids) and ids.max() >= n_c:
        raise ValueError('slates: id %d outside [0, %d)' % (ids.max(), n_c))
    if len(ids):
        rows = _csr_rows(off)
        order = np.lexsort((ids, rows))
        r, i = rows[order], ids[order]
        twice = (r[1:] == r[:-1]) & (i[1:] == i[:-1])
        if twice.any():
            w = int(np.argmax(twice))
            raise ValueError('slates: id %d repeated in slate %d' % (i[w], r[w]))
    lens = np.diff(off)
    return np.ascontiguousarray(off), np.ascontiguousarray(ids), int(lens.max()) if n else 0


_SAMPLE_BLOCK = 1 << 22             # draws held at a time by sample_negatives


def sample_negatives(users, items, eligible, seen, n_negatives, seed):
    """The slates of the sampled-negative protocol (NeuMF's: 99 negatives, HR@10 / NDCG@10; the reference's own rows,
    data.py:375-447, hold five): for row p = (users[p], items[p]) draw min(n_negatives, |pool|) DISTINCT ids uniformly
    from pool = eligible \\ seen(users[p]) \\ {items[p]}  -> the slate CSR (off int64 [n + 1], ids int64), ids ascending
    within a slate.  ``eligible``: ids (``Catalogue.eligible``); ``seen``: (off, ids), per user ascending
    (``seen_csr``).  On the host; a function of its arguments only (numpy.random.default_rng(seed)).

    Vectorised: every row takes the first n_negatives distinct pool members of 2 n_negatives + 16 uniform draws from
    ``eligible`` -- sequential rejection, so every subset of the pool is equally likely -- and only the rows that do
    not get there (a pool below n_negatives always, any other seldom) are redrawn one by one from their pool."""
    N = int(n_negatives)
    if N < 0:
        raise ValueError('sample_negatives: n_negatives = %d is negative' % N)
    u, it = _host_ints(users).reshape(-1), _host_ints(items).reshape(-1)
    if len(u) != len(it):
        raise ValueError('sample_negatives: %d users against %d items' % (len(u), len(it)))
    el = np.unique(_host_ints(eligible).reshape(-1))
    s_off, s_ids = _host_ints(seen[0]).reshape(-1), _host_ints(seen[1]).reshape(-1)
    if len(u) and (u.min() < 0 or u.max() >= len(s_off) - 1):
        raise ValueError('sample_negatives: user id outside the %d rows of seen' % (len(s_off) - 1))
    n, E = len(u), len(el)
    rng = np.random.default_rng(seed)
    lens = np.zeros(n, np.int64)
    picked = np.zeros((n, N), np.int64)
    span = int(max(el.max() if E else 0, s_ids.max() if len(s_ids) else 0, it.max() if n else 0)) + 1
    seen_keys = _csr_rows(s_off) * span + s_ids                # ascending: users in order, ids ascending within each
    redo = np.ones(n, bool)
    if N and E:
        M = 2 * N + 16
        step = max(1, _SAMPLE_BLOCK // M)
        for a in range(0, n, step):
            ub, ib = u[a:a + step], it[a:a + step]
            draw = el[rng.integers(0, E, size=(len(ub), M))]
            keys = ub[:, None] * span + draw
            at = np.searchsorted(seen_keys, keys)
            ok = (seen_keys[np.minimum(at, len(seen_keys) - 1)] != keys) if len(seen_keys) else np.ones_like(keys, bool)
            ok &= draw != ib[:, None]
            order = np.argsort(draw, axis=1, kind='stable')    # (stable: of equal ids the earliest draw comes first)
            srt = np.take_along_axis(draw, order, 1)
            again = np.zeros_like(ok)
            np.put_along_axis(again, order[:, 1:], srt[:, 1:] == srt[:, :-1], 1)
            ok &= ~again
            count = np.cumsum(ok, axis=1)
            full = count[:, -1] >= N
            take = ok & (count <= N) & full[:, None]
            picked[a:a + step][full] = np.sort(draw[take].reshape(-1, N), axis=1)
            lens[a:a + step][full] = N
            redo[a:a + step] = ~full
    slow = {}                                                  # the rows left: one by one, the pool once per user
    for p in np.nonzero(redo)[0] if N else ():
        uu = int(u[p])
        if uu not in slow:
            slow[uu] = np.setdiff1d(el, s_ids[s_off[uu]:s_off[uu + 1]])
        pool = slow[uu][slow[uu] != it[p]]
        k = min(N, len(pool))
        picked[p, :k] = pool if k == len(pool) else np.sort(rng.choice(pool, size=k, replace=False))
        lens[p] = k
    off = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=off[1:])
    return off, np.ascontiguousarray(picked[np.arange(N)[None, :] < lens[:, None]])


class Catalogue:
    """Per-item vectors and scalars of one trained model, and the top-K lists over them.

    ``refresh()`` recomputes everything cached from the model's CURRENT weights (call it again after more
    training); ``recommend`` / ``score_pairs`` read the cache.  ``engine``: the native engine training the model,
    if any -- its pending table updates are flushed first (MFEngine's blocked sweeps); the model's Parameters are
    the engines' buffers, so nothing else is read back.  A pass leaves the training state where it found it: no
    dropout draw, no step count, no conv-rule step, no token buffer of the engine is touched.

    ``towers``: 'host' (the default) builds every owner's document with numpy, copies it to the device and runs the
    tower ``tower_batch`` owners per Python call; 'device' builds the documents from the HBM-resident pools and
    enqueues the same per-chunk launches from C, one r4r_tower_span_fwd call per side and pass (csrc/tower_span.hip) --
    the same bits.  A configuration without a tower (bias_only, MF_dot, NeuMF) takes either and is unchanged."""

    _limits = staticmethod(catalogue_limits)       # a subclass names its own

    def __init__(self, model, hyper_params, train_reader, engine=None, candidates=None, tower_batch=256, towers='host'):
        if towers not in TOWERS:
            raise ValueError('catalogue: towers must be one of %r, got %r' % (TOWERS, towers))
        self.towers = towers
        why = self._limits(hyper_params)
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        self.model, self.hp, self.reader, self.engine = model, hyper_params, train_reader, engine
        self.mt = hyper_params['model_type']
        self.tower_batch = int(tower_batch)
        self.dev = next(model.parameters()).device
        if self.dev.type != 'cuda':
            raise RuntimeError('reviews4rec_amd.recommend: move the model to a ROCm device first; the HIP path has no '
                               'CPU fallback')
        self.n_users, self.n_items = int(hyper_params['total_users']), int(hyper_params['total_items'])
        self.eligible = eligible_items(hyper_params, train_reader, candidates)
        self._shape()
        self._seen = None
        self.refresh()

    def _shape(self):
        """What describes the score's form (``D``; a subclass: ``H``, ``P``, ... as its ``_head`` passes them) and
        ``n_c``, the candidate rows the kernel walks."""
        self.D = {'bias_only': 0, 'MF_dot': _latent_size(self.hp), 'deepconn': FM_RANK}[self.mt]
        # the item tables as they are (MF: total_items + 1 rows), or one per item id
        self.n_c = int(self.model.item_bias.numel()) if self.mt != 'deepconn' else self.n_items

    # ------------------------------------------------------------------ the cache
    def _flush(self):
        if self.engine is not None and hasattr(self.engine, 'flush'):
            self.engine.flush()

    def _params(self):
        return {k: v.detach() for k, v in self.model.named_parameters()}

    def _eligible_rows(self):
        """(elig, mask, ninf): the eligible ids on the device, the bool mask of their rows among the n_c candidates, and
        a fresh float32 [n_c] of -inf (the c_bias of a row that is not eligible)."""
        elig = torch.from_numpy(self.eligible).to(self.dev)
        mask = torch.zeros(self.n_c, dtype=torch.bool, device=self.dev)
        mask[elig] = True
        return elig, mask, torch.full((self.n_c,), float('-inf'), dtype=torch.float32, device=self.dev)

    def _batches(self, ids):
        """(sl, ids[sl]) over ``ids``, ``tower_batch`` at a time: token documents are dropped chunk by chunk."""
        for s in range(0, len(ids), self.tower_batch):
            sl = slice(s, s + self.tower_batch)
            yield sl, ids[sl]

    def _words(self):
        """The word table the towers read."""
        return self.model.word2vec.weight

    def _tower(self, tower, idx):
        """Eval-mode forward of a TextCNN tower (no dropout draw, no autograd): idx [n, T] -> latent [n, L]."""
        with torch.no_grad():
            conv = tower.convs[0]
            pooled, _ = ops.textcnn_fwd_raw(idx, self._words(), conv.weight.detach(), conv.bias.detach())
            return ops.linear(pooled, tower.fc.weight.detach(), tower.fc.bias.detach())

    def _documents(self, pool, ids):
        """The documents ratings outside the training split are scored with (data.py:240-246): every review of the
        owner, nothing removed, cut / zero padded to input_length."""
        from .data import _np_docs
        ids = np.asarray(ids, dtype=np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= pool.owners):
            raise KeyError('id outside the review pools: {}'.format(int(ids.max())))
        docs = _np_docs(pool.tok, pool.rev_off, pool.first[ids], pool.first[ids + 1], np.full(len(ids), -1, np.int64),
                        int(self.hp['input_length']))
        return torch.from_numpy(docs).to(self.dev)

    def _span_latents(self, tower, pool, ids, narre_pad=None, shift=0):
        """The device path of ``_tower(tower, _documents(pool, chunk))`` over every ``tower_batch`` chunk of ``ids`` (a
        host int64 array): ONE r4r_tower_span_fwd call -> latent [n, L].  ``narre_pad`` (NARRE: the pad id of the
        neighbour lists): the reviews one by one -> (latent [n R, L], neigh [n, 10]).  The id check stays on the host
        and raises before anything is enqueued; the pass has its own workspace and touches no engine buffer.
        ``shift`` > 0 (``what_if``'s slide-in slots): every owner's reviews from its ``shift``-th on, through a table of
        review ranges in which owner o is row 2 o -- [min(first[o] + shift, first[o + 1]), first[o + 1])."""
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= pool.owners):
            raise KeyError('id outside the review pools: {}'.format(int(ids.max())))
        hp, conv, n = self.hp, tower.convs[0], len(ids)
        narre = narre_pad is not None
        T = int(hp['input_length'])
        R, W = (int(hp['narre_num_reviews']), int(hp['narre_num_words'])) if narre else (0, 0)
        per = R if narre else 1
        fc_w, fc_b = ops._f32(tower.fc.weight.detach(), 'fc.weight'), ops._f32(tower.fc.bias.detach(), 'fc.bias')
        L = int(fc_w.shape[0])
        latent = torch.empty((n * per, L), dtype=torch.float32, device=self.dev)
        neigh = torch.empty((n, NEIGHBOURS), dtype=torch.int64, device=self.dev) if narre else None
        if n == 0:
            return (latent, neigh) if narre else latent
        table = ops._f32(self._words().detach(), 'table')
        conv_w, conv_b = ops._f32(conv.weight.detach(), 'conv_w'), ops._f32(conv.bias.detach(), 'conv_b')
        if table.shape[1] % 4:                                 # (ops.textcnn_fwd_raw's padding, once per pass)
            E0 = table.shape[1]
            table = ops._padded_table(self._words())
            pw = torch.zeros(tuple(conv_w.shape[:-1]) + (table.shape[1],), dtype=conv_w.dtype, device=conv_w.device)
            pw[..., :E0].copy_(conv_w)
            conv_w = pw
        V, E = (int(d) for d in table.shape)
        F = int(conv_b.numel())
        tok, rev_off, first, nb = pool.device(self.dev)
        dev_ids = torch.from_numpy(ids).to(self.dev)
        owners = int(pool.owners)
        if shift:
            ends = first[1:]
            first = torch.stack([torch.minimum(first[:-1] + int(shift), ends), ends], 1).reshape(-1)
            first, dev_ids, owners = torch.cat([first, first[-1:]]).contiguous(), dev_ids * 2, 2 * owners
        group = max(1, self.tower_batch)
        ws = ops._workspace(_lib.lib().r4r_tower_span_ws_bytes(min(group, n), T, R, W, E, F, L, V), self.dev)
        _lib.call('r4r_tower_span_fwd', ptr(tok), ptr(rev_off), ptr(first), ptr(nb), owners, ptr(dev_ids), n, group,
                  T, R, W, int(narre_pad or 0), ptr(table), V, ptr(conv_w), ptr(conv_b), ptr(fc_w), ptr(fc_b), E, F, L,
                  ptr(latent), ptr(neigh), ptr(ws), ws.numel(), None)
        return (latent, neigh) if narre else latent

    def _latents(self, tower, pool, ids):
        """(sl, ids[sl], latent [len, L]) over the ``tower_batch`` chunks of ``ids`` (a host int64 array): the tower
        forward of each chunk's documents, per chunk from the host ('host') or as slices of one span ('device')."""
        if self.towers == 'device':
            z = self._span_latents(tower, pool, ids)
            for sl, chunk in self._batches(ids):
                yield sl, chunk, z[sl]
        else:
            for sl, chunk in self._batches(ids):
                yield sl, chunk, self._tower(tower, self._documents(pool, chunk))

    def _fold(self, latent, side):
        fm, m = self.model.fm, self.model
        return fold_fm(fm.V, fm.lin.weight, fm.lin.bias, m.global_bias, latent, side)

    def refresh(self):
        self._flush()
        m = self.model
        elig, mask, ninf = self._eligible_rows()
        with torch.no_grad():
            if self.mt != 'deepconn':
                self.c = m.item_embedding.weight.detach() if self.mt == 'MF_dot' else None      # in place, not copied
                self.c_bias = torch.where(mask, m.item_bias.detach(), ninf)
                return
            c = torch.zeros((self.n_c, FM_RANK), dtype=torch.float32, device=self.dev)
            for sl, _, z in self._latents(m.item_conv, self.reader.store.items, self.eligible):
                vec, bias = self._fold(z, 'item')
                c[elig[sl]] = vec
                ninf[elig[sl]] = bias
            self.c, self.c_bias = c, ninf

    # ------------------------------------------------------------------ the query side
    def _users(self, users):
        """``users`` (a list, an array or a tensor on any device) as a host int64 tensor: the documents and the
        exclusion lists are looked up on the host."""
        u = torch.as_tensor(users, dtype=torch.int64).reshape(-1).cpu()
        if u.numel() and (int(u.min()) < 0 or int(u.max()) >= self.n_users):
            raise ValueError('catalogue: user ids must lie in [0, total_users = %d)' % self.n_users)
        return u

    def _queries(self, u_host):
        """(q [n, D] or None, q_bias [n]) of the requested users from the current weights."""
        m = self.model
        u = u_host.to(self.dev)
        with torch.no_grad():
            if self.mt != 'deepconn':
                q = m.user_embedding.weight.detach()[u].contiguous() if self.mt == 'MF_dot' else None
                return q, (m.user_bias.detach()[u] + m.global_bias.detach()).contiguous()
            q = torch.empty((u.numel(), FM_RANK), dtype=torch.float32, device=self.dev)
            qb = torch.empty((u.numel(),), dtype=torch.float32, device=self.dev)
            for sl, _, z in self._latents(m.user_conv, self.reader.store.users, u_host.numpy()):
                q[sl], qb[sl] = self._fold(z, 'user')
            return q, qb

    @property
    def seen(self):
        """(off, ids): the CSR of every user's distinct training items, built once."""
        if self._seen is None:
            self._seen = seen_csr(self.reader, self.n_users)
        return self._seen

    def _exclusions(self, u_host):
        off, ids = self.seen
        u = u_host.numpy()
        lens = off[u + 1] - off[u]
        sub_off = np.zeros(len(u) + 1, np.int64)
        np.cumsum(lens, out=sub_off[1:])
        take = np.repeat(off[u] - sub_off[:-1], lens) + np.arange(sub_off[-1], dtype=np.int64)
        sub_ids = ids[take] if len(take) else np.zeros(1, np.int64)            # (one spare entry: never a null pointer)
        return torch.from_numpy(sub_off).to(self.dev), torch.from_numpy(np.ascontiguousarray(sub_ids)).to(self.dev)

    # ------------------------------------------------------------------ the calls
    _form = 'dot'          # the entry points the calls go through: r4r_topk_<form>, r4r_pair_<form>, r4r_rank_<form>

    def _head(self, q, n, qb):
        """The leading arguments of the form's entry points: ``n`` query rows (q, q_bias), the cached item side and
        what describes the score."""
        return (ptr(q), n, ptr(qb), ptr(self.c), self.n_c, self.D, ptr(self.c_bias), self.D)

    def _pairs(self, users, items):
        """(users, items) as host int64 tensors, equally long, every id in range."""
        u = self._users(users)
        i = torch.as_tensor(items, dtype=torch.int64).reshape(-1)
        if i.numel() != u.numel():
            raise ValueError('catalogue: %d users against %d items' % (u.numel(), i.numel()))
        if i.numel() and (int(i.min()) < 0 or int(i.max()) >= self.n_c):
            raise ValueError('catalogue: item ids must lie in [0, %d)' % self.n_c)
        return u, i

    def recommend(self, users, k=10, exclude_seen=True):
        """``users``: ids as a list, a numpy array or a tensor on any device.
        -> (items int64 [n, k], scores float32 [n, k]) on the device: per user the k best eligible items, score
        descending, ties by ascending id; unused slots hold (-1, -inf).  One r4r_topk_<form> call."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError('catalogue: k = %d outside 1 .. %d' % (k, MAX_K))
        u = self._users(users)
        n = int(u.numel())
        items = torch.full((n, k), -1, dtype=torch.int64, device=self.dev)
        scores = torch.full((n, k), float('-inf'), dtype=torch.float32, device=self.dev)
        if n == 0 or self.n_c == 0:
            return items, scores
        q, qb = self._queries(u)
        eo, ei = self._exclusions(u) if exclude_seen else (None, None)
        ws_bytes = getattr(_lib.lib(), 'r4r_topk_%s_ws_bytes' % self._form)
        ws = ops._workspace(ws_bytes(n, self.n_c, k, 0), self.dev)
        _lib.call('r4r_topk_' + self._form, *self._head(q, n, qb), ptr(eo), ptr(ei), k, 0, ptr(ws), ws.numel(), ptr(items),
                  ptr(scores))
        return items, scores

    def score_pairs(self, users, items):
        """The fp32 score ``recommend`` ranks by, for explicit (user, item) pairs (lists, arrays or tensors on any
        device, equally long) -> float32 [n] on the device (-inf where the item is not eligible).  One r4r_pair_<form>
        call."""
        u, i = self._pairs(users, items)
        out = torch.empty((u.numel(),), dtype=torch.float32, device=self.dev)
        if u.numel() == 0:
            return out
        uniq, inv = torch.unique(u, return_inverse=True)
        q, qb = self._queries(uniq)
        qi, ci = inv.to(self.dev), i.to(self.dev)              # (named: the pointers must outlive the call)
        _lib.call('r4r_pair_' + self._form, *self._head(q, int(uniq.numel()), qb), ptr(qi), ptr(ci), int(u.numel()),
                  ptr(out))
        return out

    def rank(self, users, items, exclude_seen=True):
        """The place of item ``items[p]`` in the list ``recommend`` would give user ``users[p]`` if K were the whole
        catalogue (lists, arrays or tensors on any device, equally long)
        -> (ranks int64 [n], scores float32 [n]) on the device: the number of eligible items ahead of the item (score
        descending, ties by ascending id; with ``exclude_seen`` the user's training items are not counted, the item
        itself never is), -1 where the item is not eligible; the scores are ``score_pairs``' bits.  One r4r_rank_<form>
        call: no list, no sort."""
        u, i = self._pairs(users, items)
        n = int(u.numel())
        ranks = torch.full((n,), -1, dtype=torch.int64, device=self.dev)
        scores = torch.full((n,), float('-inf'), dtype=torch.float32, device=self.dev)
        if n == 0 or self.n_c == 0:
            return ranks, scores
        uniq, inv = torch.unique(u, return_inverse=True)
        q, qb = self._queries(uniq)
        eo, ei = self._exclusions(uniq) if exclude_seen else (None, None)
        qi, ti = inv.to(self.dev), i.to(self.dev)              # (named: the pointers must outlive the call)
        _lib.call('r4r_rank_' + self._form, *self._head(q, int(uniq.numel()), qb), ptr(qi), ptr(ti), n, ptr(eo), ptr(ei),
                  0, ptr(ranks), ptr(scores))
        return ranks, scores

    # ------------------------------------------------------------------ slates: a candidate list per query
    def _slates(self, slates, n):
        """``slates_csr`` of ``slates`` on the device: (off, ids, longest); ids with one spare entry (never a null
        pointer)."""
        off, ids, longest = slates_csr(slates, n, self.n_c)
        ids = np.concatenate([ids, np.zeros(1, np.int64)])
        return torch.from_numpy(off).to(self.dev), torch.from_numpy(ids).to(self.dev), longest

    def recommend_among(self, users, slates, k=10, exclude_seen=True):
        """Re-ranking: the k best of each user's OWN candidate list.  ``users``: n ids (a user may come twice, with two
        lists); ``slates``: what ``slates_csr`` takes, n rows, ids in [0, n_c).
        -> (items int64 [n, k], scores float32 [n, k]) on the device: score descending, ties by ascending id, in
        ``score_pairs``' bits; an item that is not eligible (and, with ``exclude_seen``, a training item of the user) is
        never listed; unused slots hold (-1, -inf).  One r4r_slate_topk_<form> call, queries per DISTINCT user."""
        k = int(k)
        if not 1 <= k <= MAX_K:
            raise ValueError('catalogue: k = %d outside 1 .. %d' % (k, MAX_K))
        u = self._users(users)
        n = int(u.numel())
        off, ids, longest = self._slates(slates, n)
        items = torch.full((n, k), -1, dtype=torch.int64, device=self.dev)
        scores = torch.full((n, k), float('-inf'), dtype=torch.float32, device=self.dev)
        if n == 0 or self.n_c == 0:
            return items, scores
        uniq, inv = torch.unique(u, return_inverse=True)
        q, qb = self._queries(uniq)
        eo, ei = self._exclusions(uniq) if exclude_seen else (None, None)
        qi = inv.to(self.dev)                                  # (named: the pointers must outlive the call)
        ws = ops._workspace(_lib.lib().r4r_slate_ws_bytes(n, longest, k), self.dev)
        _lib.call('r4r_slate_topk_' + self._form, *self._head(q, int(uniq.numel()), qb), ptr(qi), ptr(off), ptr(ids), n,
                  longest, ptr(eo), ptr(ei), k, ptr(ws), ws.numel(), ptr(items), ptr(scores))
        return items, scores

    def rank_among(self, users, items, slates, exclude_seen=True):
        """The sampled-negative protocol (eval.py:64-92 at any number of negatives and any K): the place of item
        ``items[p]`` among the candidates ``slates`` row p holds for user ``users[p]``
        -> (ranks int64 [n], scores float32 [n]) on the device: the number of listed items other than ``items[p]`` that
        are ahead of it (eligible ones only; with ``exclude_seen`` not the user's training items), -1 where the item
        itself is not eligible; the item need not be listed.  The scores are ``score_pairs``' bits.  One
        r4r_slate_rank_<form> call, queries per DISTINCT user."""
        u, i = self._pairs(users, items)
        n = int(u.numel())
        off, ids, longest = self._slates(slates, n)
        ranks = torch.full((n,), -1, dtype=torch.int64, device=self.dev)
        scores = torch.full((n,), float('-inf'), dtype=torch.float32, device=self.dev)
        if n == 0 or self.n_c == 0:
            return ranks, scores
        uniq, inv = torch.unique(u, return_inverse=True)
        q, qb = self._queries(uniq)
        eo, ei = self._exclusions(uniq) if exclude_seen else (None, None)
        qi, ti = inv.to(self.dev), i.to(self.dev)              # (named: the pointers must outlive the call)
        _lib.call('r4r_slate_rank_' + self._form, *self._head(q, int(uniq.numel()), qb), ptr(qi), ptr(ti), ptr(off),
                  ptr(ids), n, longest, ptr(eo), ptr(ei), ptr(ranks), ptr(scores))
        return ranks, scores

    # ------------------------------------------------------------------ phrase explanations: the windows that win the pool
    def _phrase_side(self, side):
        """(pool, TextCNN tower, NARRE's neighbour pad id or None) of 'user' / 'item'; a configuration without a tower
        is refused with the reason."""
        why = phrase_limits(self.hp)
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        m = self.model
        return (self.reader.store.users, m.user_conv, None) if side == 'user' else (self.reader.store.items, m.item_conv, None)

    def _phrase_weights(self, tower, weights, n, per):
        """``explain_words``' ``weights`` as what the kernel takes: None, [F] or one row per document [n per, F].  NARRE
        (``per`` = R > 1) also takes one row per REVIEW, [n, R, F]."""
        F = int(tower.convs[0].bias.numel())
        if weights is None:
            return None
        if isinstance(weights, str):
            if weights != 'latent':
                raise ValueError("catalogue: weights must be None, 'latent' or a tensor [F] / [n, F], got %r" % (weights,))
            return tower.fc.weight.detach().norm(dim=0).to(torch.float32).contiguous()
        shapes = ((F,), (n, F)) + (((n, per, F),) if per > 1 else ())
        if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or tuple(weights.shape) not in shapes:
            raise ValueError("catalogue: weights must be None, 'latent' or a float32 tensor [%d] / [%d, %d]%s, got %s"
                             % (F, n, F, ' / [%d, %d, %d]' % (n, per, F) if per > 1 else '',
                                tuple(weights.shape) if isinstance(weights, torch.Tensor) else type(weights).__name__))
        weights = weights.detach().to(self.dev).contiguous()
        if weights.dim() == 3:
            return weights.reshape(n * per, F)                 # a row per review already
        if weights.dim() == 2 and per > 1:
            weights = weights.repeat_interleave(per, dim=0).contiguous()      # an owner's row for each of its reviews
        return weights

    def _phrase_rows(self, tower, pool, ids, k, wt, narre_pad=None):
        """r4r_textcnn_phrases over the documents of ``ids`` (a host int64 array; NARRE: over each owner's R reviews)
        -> (positions, scores, filters, tokens, windows), one row per document.  'host': numpy documents and one
        textcnn_fwd_raw + textcnn_phrases call per ``tower_batch`` owners; 'device': ONE r4r_tower_span_phrases call,
        the same bits."""
        hp, conv, n = self.hp, tower.convs[0], len(ids)
        narre = narre_pad is not None
        T = int(hp['narre_num_words']) if narre else int(hp['input_length'])
        R = int(hp['narre_num_reviews']) if narre else 0
        per = R if narre else 1
        rows = n * per
        i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=self.dev)
        pos, filt, win = i32(rows, k), i32(rows, k), i32(rows)
        score = torch.empty((rows, k), dtype=torch.float32, device=self.dev)
        tokens = torch.empty((rows, k, 3), dtype=torch.int64, device=self.dev)
        if n == 0:
            return pos, score, filt, tokens, win
        per_row = wt is not None and wt.dim() == 2
        if self.towers != 'device':
            from .data import _np_reviews
            for sl, chunk in self._batches(ids):
                if narre:
                    none = np.full(len(chunk), -1, np.int64)
                    docs = _np_reviews(pool.tok, pool.rev_off, pool.first[chunk], pool.first[chunk + 1], none, R, T)
                    docs = torch.from_numpy(docs.reshape(len(chunk) * R, T)).to(self.dev)
                else:
                    docs = self._documents(pool, chunk)
                rs = slice(sl.start * per, sl.start * per + len(chunk) * per)
                pooled, argmax = ops.textcnn_fwd_raw(docs, self._words(), conv.weight.detach(), conv.bias.detach())
                pos[rs], score[rs], filt[rs], tokens[rs], win[rs] = ops.textcnn_phrases(
                    pooled, argmax, k, T, weights=wt[rs] if per_row else wt, idx=docs)
            return pos, score, filt, tokens, win
        table = ops._f32(self._words().detach(), 'table')
        conv_w, conv_b = ops._f32(conv.weight.detach(), 'conv_w'), ops._f32(conv.bias.detach(), 'conv_b')
        if table.shape[1] % 4:                                 # (ops.textcnn_fwd_raw's padding, once per pass)
            E0 = table.shape[1]
            table = ops._padded_table(self._words())
            pw = torch.zeros(tuple(conv_w.shape[:-1]) + (table.shape[1],), dtype=conv_w.dtype, device=conv_w.device)
            pw[..., :E0].copy_(conv_w)
            conv_w = pw
        V, E = (int(d) for d in table.shape)
        F, L = int(conv_b.numel()), int(tower.fc.weight.shape[0])
        tok, rev_off, first, nb = pool.device(self.dev)
        dev_ids = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int64)).to(self.dev)
        neigh = torch.empty((n, NEIGHBOURS), dtype=torch.int64, device=self.dev) if narre else None
        group = max(1, self.tower_batch)
        ws = ops._workspace(_lib.lib().r4r_tower_span_ws_bytes(min(group, n), 0 if narre else T, R, T if narre else 0, E, F,
                                                               L, V), self.dev)
        _lib.call('r4r_tower_span_phrases', ptr(tok), ptr(rev_off), ptr(first), ptr(nb), int(pool.owners), ptr(dev_ids), n,
                  group, 0 if narre else T, R, T if narre else 0, int(narre_pad or 0), ptr(table), V, ptr(conv_w),
                  ptr(conv_b), E, F, ptr(wt), F if per_row else 0, k, ptr(pos), ptr(score), ptr(filt), ptr(tokens),
                  ptr(win), ptr(neigh), ptr(ws), ws.numel(), None)
        return pos, score, filt, tokens, win

    def _phrase_request(self, ids, k, side, weights, per=1):
        """``explain_words``' checks, in order, before anything runs -> (ids as a host array, pool, tower, pad, wt)."""
        if side not in ('item', 'user'):
            raise ValueError("catalogue: side must be 'item' or 'user', got %r" % (side,))
        pool, tower, pad = self._phrase_side(side)
        F = int(tower.convs[0].bias.numel())
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= F:
            raise ValueError('catalogue: explain_words k = %r outside 1 .. %d' % (k, F))
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu().numpy()
        wt = self._phrase_weights(tower, weights, len(ids), per)
        if len(ids) and (ids.min() < 0 or ids.max() >= pool.owners):
            raise KeyError('id outside the review pools: {}'.format(int(ids.max())))
        return ids, pool, tower, pad, wt

    def explain_words(self, ids, k=5, side='item', weights=None):
        """The phrases that carry an owner's latent vector: per item (``side='item'``; 'user': per user) the ``k``
        heaviest three-word windows of its document, i.e. the windows that won the max-pool of the side's TextCNN tower
        (common_pytorch_models.py:29-31; include/r4r.h, "Phrase explanations"), from the current weights
        -> ``Phrases`` of device tensors, n = len(ids):

            positions  int32 [n, k]     the window's conv position p: it covers the words p - 2 .. p; fill -1
            scores     float32 [n, k]   the window's weight, descending, ties by ascending position; fill 0
            filters    int32 [n, k]     the number of filters whose maximum the window is; fill 0
            tokens     int64 [n, k, 3]  the window's word ids; -1 in the conv's zero padding and in a fill entry
            reviews    int64 [n, k]     the index in that side's pool of the review holding the window's first
                                        in-document token (``pool.rev_off`` / ``pool.tok`` give its tokens); -1 for a
                                        window that lies wholly in padding
            offsets    int64 [n, k]     that token's word offset inside the review; -1 with reviews == -1
            windows    int32 [n]        the number of distinct windows of the owner

        ``weights``: None -- a window's score is the activation mass it won, the sum of its filters' pooled values;
        'latent' -- each filter weighed by ``tower.fc.weight.norm(dim=0)``, how far a unit of the feature moves the
        latent vector; a float32 tensor [F] or [n, F] -- the caller's own, e.g. the gradient of a pair's score.
        One r4r_textcnn_phrases call per ``tower_batch`` chunk ('host') or one r4r_tower_span_phrases call ('device'):
        the same bits.  An id outside the side's pool raises KeyError; ``k`` outside 1 .. F, a bad ``side`` and bad
        ``weights`` raise ValueError; a configuration without a tower is refused with the reason.  The engine's pending
        updates are flushed first, as ``refresh()`` does; the training state is left untouched."""
        ids, pool, tower, _, wt = self._phrase_request(ids, k, side, weights)
        k = int(k)
        self._flush()
        with torch.no_grad():
            pos, score, filt, tokens, win = self._phrase_rows(tower, pool, ids, k, wt)
        _, rev_off, first, _ = pool.device(self.dev)
        own = torch.from_numpy(ids).to(self.dev)
        begin, end = rev_off[first[own]], rev_off[first[own + 1]]                 # the owner's tokens in the pool
        t0 = (pos.to(torch.int64) - 2).clamp(min=0)                              # the first in-document word (p < T + 2)
        at = begin[:, None] + t0
        inside = (pos >= 0) & (at < end[:, None])
        review = torch.searchsorted(rev_off, at.contiguous(), right=True) - 1
        minus = torch.full_like(at, -1)
        reviews = torch.where(inside, review, minus)
        offsets = torch.where(inside, at - rev_off[review.clamp(min=0, max=rev_off.numel() - 1)], minus)
        return Phrases(pos, score, filt, tokens, reviews, offsets, win)

    # ------------------------------------------------------------------ pair explanations: the words behind ONE score
    _pair_kind = 'fm'      # r4r_pair_grad's kind for this class's head (ops.PAIR_GRAD_KINDS)

    def _pair_limits(self):
        """None when ``pair_weights`` / ``explain_pair`` serve this configuration, else the reason."""
        return phrase_limits(self.hp)

    def _pair_head(self, u, i):
        """The RAW head parameters ``ops.pair_grad`` takes for this class's kind, with the score's scalars of the users
        ``u`` / the items ``i`` (device int64, the rows of zu / zi) summed in float64 and rounded once.  deepconn
        (DeepCoNN.py:61-66): the FM over [user | item]; lin.bias and the global bias are the only scalars."""
        m = self.model
        f64 = lambda t: t.detach().to(torch.float64).reshape(())
        qb = (f64(m.fm.lin.bias) + f64(m.global_bias)).to(torch.float32)
        return dict(V=m.fm.V.detach(), lw=m.fm.lin.weight.detach().reshape(-1), q_bias=qb.expand(u.numel()).contiguous())

    def _pair_request(self, users, items):
        """``pair_weights``' checks of the ids, before anything runs -> (users, items) as host int64 tensors: equally
        long, every id an owner of its side's review pool."""
        u = torch.as_tensor(users, dtype=torch.int64).reshape(-1).cpu()
        i = torch.as_tensor(items, dtype=torch.int64).reshape(-1).cpu()
        if i.numel() != u.numel():
            raise ValueError('catalogue: %d users against %d items' % (u.numel(), i.numel()))
        for ids, side in ((u, 'user'), (i, 'item')):
            pool = self._phrase_side(side)[0]
            if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= pool.owners):
                raise KeyError('id outside the review pools: {}'.format(int(ids.max())))
        return u, i

    def _pair_weights(self, u, i):
        """``pair_weights`` of checked host id tensors: the towers of the DISTINCT users and items through ``_latents``,
        then ONE r4r_pair_grad call."""
        self._flush()
        (pool_u, tower_u, _), (pool_i, tower_i, _) = self._phrase_side('user'), self._phrase_side('item')
        fc_u, fc_i = tower_u.fc.weight.detach(), tower_i.fc.weight.detach()
        L, F = (int(d) for d in fc_u.shape)
        n = int(u.numel())
        if n == 0:
            none = torch.empty((0, F), dtype=torch.float32, device=self.dev)
            return none, none.clone(), torch.empty((0,), dtype=torch.float32, device=self.dev)
        uu, u_inv = torch.unique(u, return_inverse=True)
        ui, i_inv = torch.unique(i, return_inverse=True)
        with torch.no_grad():
            zu = torch.empty((uu.numel(), L), dtype=torch.float32, device=self.dev)
            zi = torch.empty((ui.numel(), L), dtype=torch.float32, device=self.dev)
            for sl, _, z in self._latents(tower_u, pool_u, uu.numpy()):
                zu[sl] = z
            for sl, _, z in self._latents(tower_i, pool_i, ui.numpy()):
                zi[sl] = z
            out = ops.pair_grad(self._pair_kind, zu, zi, u_inv.to(self.dev), i_inv.to(self.dev), fc_u=fc_u, fc_i=fc_i,
                                want=('score', 'w_user', 'w_item'), **self._pair_head(uu.to(self.dev), ui.to(self.dev)))
        return out['w_user'], out['w_item'], out['score']

    def pair_weights(self, users, items):
        """Why THIS item for THIS user: for the pairs (users[p], items[p]) (lists, arrays or tensors on any device,
        equally long; owners of the review pools, with or without a training rating)
        -> (w_user float32 [n, F], w_item float32 [n, F], scores float32 [n]) on the device:

            w_user[p, f]   d score(users[p], items[p]) / d pooled_f of the user tower: how much a unit of filter f's
                           max-pooled activation moves the pair's predicted rating; w_item: the same of the item tower
            scores[p]      the model's eval-mode prediction for the pair, from the raw head parameters (``score_pairs``
                           reads the catalogue's folds: the same number by another fp32 chain, and -inf for an item
                           that is not eligible, which this call does not look at)

        The rows are what ``explain_words(..., weights=)`` takes.  The towers of the distinct users and items run once
        through ``_latents`` (``towers`` 'host' and 'device': the same bits), then ONE r4r_pair_grad call (include/r4r.h,
        "Pair gradients") over the model's current weights.  The engine's pending updates are flushed first, as
        ``refresh()`` does; the training state is left untouched.  Unequal lengths raise ValueError, an id outside its
        side's pool KeyError; a configuration without a tower is refused with the reason.  NARRE is refused here too: its
        answer is per review and lives under ``NarreCatalogue.pair_reviews`` / ``explain_pair_reviews``."""
        why = self._pair_limits()
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        return self._pair_weights(*self._pair_request(users, items))

    def explain_pair(self, users, items, k=5, direction='up'):
        """The words behind one user-item score: for every pair, the ``k`` three-word windows of the USER's reviews and
        the ``k`` windows of the ITEM's reviews that move the pair's predicted rating most
        -> ``PairPhrases(user, item, scores)``: ``user`` is ``explain_words(users, k, 'user', weights=+-w_user)`` and
        ``item`` is ``explain_words(items, k, 'item', weights=+-w_item)`` of ``pair_weights(users, items)``, bit for
        bit (they are made by those calls), and ``scores`` its scores.  ``direction``: 'up' lists the windows that
        RAISE the prediction most (+w: a window's score is the first-order change of the rating per unit of its
        filters' activations, times those activations), 'down' the ones that lower it most (-w).  A window score below
        zero under 'up' is a window that lowers the rating: the lists are sorted, not cut at zero.  Refusals as
        ``pair_weights``', then a ``direction`` other than 'up' / 'down', ``k`` outside 1 .. F, unequal lengths
        (ValueError) and an id outside its side's pool (KeyError), before anything is enqueued."""
        why = self._pair_limits()
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        if direction not in ('up', 'down'):
            raise ValueError("catalogue: direction must be 'up' or 'down', got %r" % (direction,))
        F = int(self._phrase_side('item')[1].convs[0].bias.numel())
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= F:
            raise ValueError('catalogue: explain_pair k = %r outside 1 .. %d' % (k, F))
        u, i = self._pair_request(users, items)
        w_user, w_item, scores = self._pair_weights(u, i)
        if direction == 'down':
            w_user, w_item = -w_user, -w_item
        return PairPhrases(self.explain_words(u, k=int(k), side='user', weights=w_user),
                           self.explain_words(i, k=int(k), side='item', weights=w_item), scores)

    # ------------------------------------------------------------------ what-if scores: reviews or words REMOVED
    pair_batch = 8192      # pairs per r4r_pair_grad call of the what-if passes; set after construction
    whatif_rows = (0, 0)   # the variant rows (user side, item side) the last what-if pass sent through the towers

    def _whatif_slots(self, pool, own):
        """Of the first 64 reviews of the owners ``own`` -> (has, seen) bool [len(own), 64]: the slot holds a review; and
        the review shows in the base document (it is not empty and starts before input_length) -- removing one that
        does not, alone or with others like it, leaves the document as it is."""
        T = int(self.hp['input_length'])
        rb, count = pool.first[own], pool.first[own + 1] - pool.first[own]
        s = np.arange(WHATIF_MAX_SLOTS, dtype=np.int64)[None, :]
        has = s < count[:, None]
        at = pool.rev_off[np.where(has, rb[:, None] + s, 0)]
        return has, has & (pool.rev_off[np.where(has, rb[:, None] + s + 1, 0)] > at) & (at - pool.rev_off[rb][:, None] < T)

    def _loo_rows(self, pool, ids, S):
        """``_whatif_rows`` for ``leave_one_out``'s masks -- variant s of a pair removes its owner's review s, s < S --
        from the DISTINCT owners alone, without a pass over the pairs' variants."""
        own, inv = np.unique(ids, return_inverse=True)
        nb = len(own)
        _, seen = self._whatif_slots(pool, own)
        starts = nb + np.concatenate([[0], np.cumsum(seen.sum(1))[:-1]]).astype(np.int64)
        row = np.where(seen, starts[:, None] + np.cumsum(seen, 1) - 1, np.arange(nb, dtype=np.int64)[:, None])
        o, slot = np.nonzero(seen)                              # (row-major: the order of the rows numbered above)
        row_ids = np.concatenate([own, own[o]])
        row_drop = np.concatenate([np.zeros(nb, np.int64), (np.uint64(1) << slot.astype(np.uint64)).view(np.int64)])
        return row_ids, row_drop, None, np.concatenate([inv[:, None], row[inv][:, :S]], 1), nb

    def _whatif_rows(self, pool, ids, masks, occ):
        """One side's variants as DISTINCT tower rows.  ``ids``: host int64 [n]; ``masks``: int64 [n, V] or None;
        ``occ``: int64 [n, V, P] (-1 unused) or None -> (row_ids [M], row_drop [M], row_occ [M, P] or None,
        index [n, V + 1], n_base): rows 0 .. n_base - 1 are the distinct owners with nothing removed, the rest the
        distinct (owner, mask, positions); ``index[p, 0]`` is pair p's base row and ``index[p, 1 + v]`` variant v's.
        A mask's bits at or beyond min(count, 64) are cleared; a mask every dropped review of which is empty or starts
        at or beyond T leaves the document as it is and becomes 0; positions are sorted, repeats dropped.  A variant
        with nothing left to remove IS its owner's base row."""
        own, inv = np.unique(ids, return_inverse=True)
        n, nb = len(ids), len(own)
        V = masks.shape[1] if masks is not None else (occ.shape[1] if occ is not None else 0)
        index = np.empty((n, V + 1), np.int64)
        index[:, 0] = inv
        if V == 0 or n == 0:
            return own, np.zeros(nb, np.int64), None, index, nb
        s = np.arange(WHATIF_MAX_SLOTS, dtype=np.int64)[None, :]
        has, seen = self._whatif_slots(pool, own)
        pack = lambda b: (b.astype(np.uint64) << s.astype(np.uint64)).sum(1, dtype=np.uint64).view(np.int64)
        m = np.zeros((n, V), np.int64) if masks is None else masks & pack(has)[inv][:, None]
        m = np.where((m & pack(seen)[inv][:, None]) != 0, m, 0)
        P = occ.shape[2] if occ is not None else 0
        key = np.empty((n * V, 2 + P), np.int64)
        key[:, 0], key[:, 1] = np.repeat(inv, V), m.reshape(-1)
        if P:
            o = np.sort(occ.reshape(n * V, P), axis=1)
            o[:, 1:][o[:, 1:] == o[:, :-1]] = -1                                 # repeats
            key[:, 2:] = -np.sort(-o, axis=1)                                    # descending: the -1 fill at the tail
        plain = (key[:, 1:] == np.array([0] + [-1] * P)).all(1)
        rows, where = (np.unique(key[~plain], axis=0, return_inverse=True) if not plain.all() else
                       (np.zeros((0, 2 + P), np.int64), np.zeros(0, np.int64)))
        flat = np.empty(n * V, np.int64)
        flat[plain], flat[~plain] = key[plain, 0], nb + where.reshape(-1)
        index[:, 1:] = flat.reshape(n, V)
        row_ids = np.concatenate([own, own[rows[:, 0]]])
        row_drop = np.concatenate([np.zeros(nb, np.int64), rows[:, 1]])
        row_occ = np.concatenate([np.full((nb, P), -1, np.int64), rows[:, 2:]]) if P else None
        return row_ids, row_drop, row_occ, index, nb

    def _whatif_latents(self, tower, pool, row_ids, row_drop, row_occ):
        """The tower over variant rows -> latent [M, L], ``tower_batch`` rows per round: numpy documents
        (``data._np_docs_masked``) and ``_tower`` per chunk ('host'), or ONE r4r_tower_span_variants call ('device') --
        the same bits."""
        T = int(self.hp['input_length'])
        conv, M = tower.convs[0], len(row_ids)
        if self.towers != 'device' or M == 0:
            from .data import _np_docs_masked
            z = torch.empty((M, int(tower.fc.weight.shape[0])), dtype=torch.float32, device=self.dev)
            for sl, chunk in self._batches(row_ids):
                docs = _np_docs_masked(pool.tok, pool.rev_off, pool.first[chunk], pool.first[chunk + 1], row_drop[sl],
                                       None if row_occ is None else row_occ[sl], T)
                z[sl] = self._tower(tower, torch.from_numpy(docs).to(self.dev))
            return z
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        occ_off = occ_pos = None
        if row_occ is not None:
            used = row_occ >= 0
            off = np.zeros(M + 1, np.int64)
            np.cumsum(used.sum(1), out=off[1:])
            occ_off, occ_pos = dev(off), dev(row_occ[used].astype(np.int32))
        return ops.tower_span_variants(pool.device(self.dev), dev(row_ids), T, self._words().detach(), conv.weight.detach(),
                                       conv.bias.detach(), tower.fc.weight.detach(), tower.fc.bias.detach(),
                                       max(1, self.tower_batch), drop=dev(row_drop), occ_off=occ_off, occ_pos=occ_pos)

    def _whatif_request(self, users, items):
        """The checks every what-if call starts with -> (u, i) as host int64 arrays."""
        why = phrase_limits(self.hp)
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        u, i = self._pair_request(users, items)
        return u.numpy(), i.numpy()

    def _what_if(self, u, i, mask_u, mask_i, occ_u, occ_i):
        """``what_if`` of checked host arrays -> (scores [n, V], base [n], same [n, V]): ``same`` marks the variants
        that ARE the base on both sides; their scores are the base's bits."""
        (pool_u, tower_u, _), (pool_i, tower_i, _) = self._phrase_side('user'), self._phrase_side('item')
        n = len(u)
        V = next((int(t.shape[1]) for t in (mask_u, mask_i, occ_u, occ_i) if t is not None), 1)
        if n == 0:
            e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=self.dev)
            return e(0, V), e(0), e(0, V, dt=torch.bool)
        self._flush()
        fill = lambda m, o: (np.zeros((n, V), np.int64), None) if m is None and o is None else (m, o)
        return self._whatif_scores(self._whatif_rows(pool_u, u, *fill(mask_u, occ_u)),
                                   self._whatif_rows(pool_i, i, *fill(mask_i, occ_i)))

    def _whatif_scores(self, rows_u, rows_i):
        """The towers over both sides' distinct rows (``_whatif_rows``' tuples), then the pairs' variants through
        r4r_pair_grad, ``pair_batch`` pairs per call -> (scores [n, V], base [n], same [n, V])."""
        (pool_u, tower_u, _), (pool_i, tower_i, _) = self._phrase_side('user'), self._phrase_side('item')
        (ru, du, ou, xu, bu), (ri, di, oi, xi, bi) = rows_u, rows_i
        n, V = xu.shape[0], xu.shape[1] - 1
        self.whatif_rows = (len(ru) - bu, len(ri) - bi)          # the variant rows the last pass ran, per side
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        with torch.no_grad():
            if self.fold and ou is None and oi is None:     # no occlusion: no document is built, no tower runs
                zu, zi = self._fold_latents(tower_u, pool_u, ru, du), self._fold_latents(tower_i, pool_i, ri, di)
            else:
                zu = self._whatif_latents(tower_u, pool_u, ru, du, ou)
                zi = self._whatif_latents(tower_i, pool_i, ri, di, oi)
            head = self._pair_head(dev(ru), dev(ri))
            out = torch.empty((n, V + 1), dtype=torch.float32, device=self.dev)
            same = torch.empty((n, V), dtype=torch.bool, device=self.dev)
            step = max(1, int(self.pair_batch))
            for s0 in range(0, n, step):
                sl = slice(s0, s0 + step)
                out[sl] = ops.pair_grad(self._pair_kind, zu, zi, dev(xu[sl]).reshape(-1), dev(xi[sl]).reshape(-1),
                                        want=('score',), **head)['score'].view(-1, V + 1)
                same[sl] = dev((xu[sl, 1:] < bu) & (xi[sl, 1:] < bi))
            base = out[:, 0].contiguous()
            return torch.where(same, base[:, None], out[:, 1:]).contiguous(), base, same

    def what_if(self, users, items, drop_user=None, drop_item=None, occlude_user=None, occlude_item=None):
        """What would the model predict for (users[p], items[p]) if chosen reviews, or chosen words, were not there?
        -> ``WhatIf(scores [n, V], base [n])`` of device tensors: ``scores[p, v]`` is the eval-mode prediction with
        variant v's removals applied to the user's and / or the item's document, ``base[p]`` the prediction with
        nothing removed.

        ``drop_user`` / ``drop_item``: None; or, per pair, a list of review indices in the owner's pool order -- the
        loader's ``skip`` (data.py:223-235), generalised to a set: the remaining reviews are concatenated and cut /
        padded to input_length, so later words slide in across the cut -- as one variant, or a list of such lists as V
        variants; or an int64 mask tensor [n, V], bit s = the owner's review s removed (bits beyond the owner's list are
        ignored).  Only an owner's first 64 reviews can be removed.  ``occlude_user`` / ``occlude_item``: None; an int
        tensor [n, V, P] of document positions, -1 unused; or per pair a list of positions (one variant) or a list of
        such lists.  An occluded position holds word 0, the padding the model knows, with no shift; positions refer to
        the variant's OWN document, i.e. after its removals.  All four combine; every one given has the same V.

        A variant is a document: the DISTINCT (owner, mask, positions) go through the side's tower once,
        ``tower_batch`` rows per round -- numpy documents per chunk ('host') or ONE r4r_tower_span_variants call
        ('device'; include/r4r.h, "What-if documents"): the same bits -- and the variants' latents stand in for their
        owners' in ONE r4r_pair_grad pass, ``pair_batch`` pairs at a time, over the class's own head.  Before the
        engine is flushed or anything is enqueued: a configuration without a tower is refused with the reason; unequal
        lengths, unequal V, a malformed argument, a review index outside the owner's list or at or beyond 64 and a
        position outside [0, input_length) raise ValueError, an id outside its side's pool KeyError."""
        u, i = self._whatif_request(users, items)
        T = int(self.hp['input_length'])
        args = []
        for ids, side, drop, occ in ((u, 'user', drop_user, occlude_user), (i, 'item', drop_item, occlude_item)):
            pool = self._phrase_side(side)[0]
            args += [_drop_masks(drop, pool.first[ids + 1] - pool.first[ids], 'drop_' + side),
                     _occlusions(occ, len(ids), T, 'occlude_' + side)]
        vs = sorted({int(a.shape[1]) for a in args if a is not None})
        if len(vs) > 1:
            raise ValueError('catalogue: what_if arguments hold %s variants per pair; every one needs as many' % vs)
        scores, base, _ = self._what_if(u, i, args[0], args[2], args[1], args[3])
        return WhatIf(scores, base)

    def leave_one_out(self, users, items):
        """Each review of each pair's two documents removed in turn -> ``DocLeaveOneOut`` of device tensors:

            base                          float32 [n]      the prediction with nothing removed
            without_user, without_item    float32 [n, S]   the prediction without the owner's s-th review (the loader's
                                                           ``skip`` = s); S = the side's largest ``live``
            delta_user, delta_item        float32 [n, S]   base - without: what review s adds to THIS pair's score
            live_user, live_item          int64 [n]        min(number of reviews, 64): the slots that hold a review
            reach_user, reach_item        int64 [n]        the reviews that start before position input_length of the
                                                           base document (a later one cannot show in it)

        A slot at or beyond ``live`` holds ``base`` and a delta of exactly 0; so does every slot whose review is empty
        or starts at or beyond input_length: its document IS the base document, and it is not run.  Variant rows depend
        on the owner alone: every distinct (owner, review) goes through the tower once.  One ``what_if`` pass; its
        checks and refusals."""
        u, i = self._whatif_request(users, items)
        n, T = len(u), int(self.hp['input_length'])
        sides = []
        for ids, side in ((u, 'user'), (i, 'item')):
            pool = self._phrase_side(side)[0]
            rb, count = pool.first[ids], pool.first[ids + 1] - pool.first[ids]
            live = np.minimum(count, WHATIF_MAX_SLOTS)
            cut = pool.rev_off[rb] + T                          # reviews starting before it: a prefix of the owner's list
            reach = np.searchsorted(pool.rev_off[:-1], cut, side='left') - rb if len(pool.rev_off) > 1 else np.zeros(n, np.int64)
            sides.append((live, np.clip(reach, 0, count), int(live.max()) if n else 0))
        (live_u, reach_u, S_u), (live_i, reach_i, S_i) = sides
        if n and S_u + S_i:
            self._flush()
            ru, du, _, xu, bu = self._loo_rows(self._phrase_side('user')[0], u, S_u)
            ri, di, _, xi, bi = self._loo_rows(self._phrase_side('item')[0], i, S_i)
            xu = np.concatenate([xu, np.repeat(xu[:, :1], S_i, 1)], 1)           # variants: the user's slots, then the item's
            xi = np.concatenate([xi[:, :1], np.repeat(xi[:, :1], S_u, 1), xi[:, 1:]], 1)
            scores, base, _ = self._whatif_scores((ru, du, None, xu, bu), (ri, di, None, xi, bi))
        else:
            scores, base, _ = self._what_if(u, i, None, None, None, None)
            scores = scores[:, :0]
        held = lambda S: base[:, None].expand(n, S)
        wu, wi = scores[:, :S_u].contiguous(), scores[:, S_u:].contiguous()
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.dev)
        return DocLeaveOneOut(base, wu, wi, held(S_u) - wu, held(S_i) - wi, dev(live_u), dev(live_i), dev(reach_u),
                              dev(reach_i))

    def _leave_topk_targets(self, u, i, k):
        """``counterfactual``'s ``k``: per pair the score of the k-th best eligible unseen OTHER item of the user, from
        ``recommend(users, k + 1)`` over the distinct users; -inf where the user has fewer than k other items."""
        uu, inv = torch.unique(u, return_inverse=True)
        items, scores = self.recommend(uu, k + 1)
        items, scores = items[inv.to(self.dev)], scores[inv.to(self.dev)]
        other = items != i.to(self.dev)[:, None]               # the item itself steps aside; its place goes to the next
        place = torch.cumsum(other.to(torch.int64), 1)
        at = ((place == k) & other).to(torch.int64).argmax(1)
        has = ((place == k) & other).any(1) & (items.gather(1, at[:, None])[:, 0] >= 0)
        got = scores.gather(1, at[:, None])[:, 0]
        return torch.where(has, got, torch.full_like(got, float('-inf'))).contiguous()

    # ------------------------------------------------------------------ the document fold: variants without documents
    fold = False           # True: what_if / leave_one_out without occlusion go through the fold, not the towers

    def _fold_side(self, tower, pool, own, ptab=None):
        """What ``ops.fold_latents`` / ``ops.fold_search`` take for one side: the tower's projected table (one
        r4r_fold_project unless ``ptab`` is handed in) and the interior maxima of the reviews of the DISTINCT owners
        ``own`` (a host int64 array), S = their largest min(count, 64)."""
        conv = tower.convs[0]
        if ptab is None:
            ptab = ops.fold_project(self._words().detach(), conv.weight.detach())
        live = np.minimum(pool.first[own + 1] - pool.first[own], WHATIF_MAX_SLOTS)
        ids = torch.from_numpy(np.ascontiguousarray(own, dtype=np.int64)).to(self.dev)
        pd = pool.device(self.dev)
        seg = ops.fold_segments(ptab, conv.bias.detach(), pd, ids, max(1, int(live.max()) if len(own) else 1))
        return dict(ptab=ptab, conv_b=conv.bias.detach(), seg=seg, pool=pd, ids=ids, fc_w=tower.fc.weight.detach(),
                    fc_b=tower.fc.bias.detach())

    def _fold_latents(self, tower, pool, row_ids, row_drop):
        """``_whatif_latents`` without occlusion, by the fold (include/r4r.h, "Document fold"): project, segments over
        the distinct owners, compose and the tower's fc -> latent [M, L]."""
        own, inv = np.unique(row_ids, return_inverse=True)
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.dev)
        return ops.fold_latents(self._fold_side(tower, pool, own), dev(inv), int(self.hp['input_length']),
                                drop=dev(row_drop))

    def shapley(self, *args, **kw):
        """Refused: exact Shapley values are ``NarreCatalogue.shapley``'s.  NARRE reads its reviews one by one, so a
        coalition of reviews is a re-selection of slots; here a coalition is a new document and a tower forward."""
        raise RuntimeError('reviews4rec_amd.recommend: shapley needs the score of every coalition of reviews; model_type '
                           '%r reads one document per owner, so a coalition there is a new document and a tower forward '
                           '(2^n of them per pair): use leave_one_out. NarreCatalogue.shapley is exact because a NARRE '
                           'review enters the score through its own latent and logit alone' % (self.hp.get('model_type'),))

    def review_counterfactual(self, users, items, target=None, k=None, direction='down', side='both', budget=5):
        """Which reviews would have to be missing from the user's and / or the item's document for the model to stop
        predicting ``target`` for (users[p], items[p]), and how few are enough?  ``NarreCatalogue.counterfactual``'s
        greedy search for the families whose towers read one document per owner (deepconn, deepconn++, the TransNets):
        at each step every review that SHOWS in the current document of the chosen side(s) -- it is not empty and
        starts before input_length -- is removed in turn (the loader's removal, as ``what_if``: later words slide in),
        the removal that moves the score furthest in ``direction`` is kept, even when it moves the score the wrong
        way, and the search ends when the score has passed the target, after ``budget`` removals, or when no such
        review is left -> ``Counterfactual`` of device tensors, its fields as ``NarreCatalogue.counterfactual``
        documents them.  Only an owner's first 64 reviews can be removed.

        ``target`` / ``k`` / ``direction`` / ``side``: ``NarreCatalogue.counterfactual``'s, with its checks; ``k`` goes
        with ``side='item'`` and ``direction='down'`` only.  ``budget``: 1 .. 64.  No document is built and no tower
        runs: per call one r4r_fold_project per side, per ``pair_batch`` pairs the interior maxima of the distinct
        owners' reviews (r4r_fold_segments) and ``budget`` steps of fixed shape enqueued without a host read in between
        (``ops.fold_search``; include/r4r.h, "Document fold").  Every score is ``what_if``'s score of the same removals
        with ``fold = True``, bit for bit; the results do not depend on the batch.  The greedy answer is an upper bound
        of the fewest removals, not the minimum.  The engine's pending updates are flushed first; the training state is
        left untouched."""
        why = phrase_limits(self.hp)
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        if side not in ('user', 'item', 'both'):
            raise ValueError("catalogue: side must be 'user', 'item' or 'both', got %r" % (side,))
        if direction not in ('up', 'down'):
            raise ValueError("catalogue: direction must be 'up' or 'down', got %r" % (direction,))
        if (target is None) == (k is None):
            raise ValueError('catalogue: counterfactual takes exactly one of target and k, got target = %r and k = %r'
                             % (target, k))
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K - 1:
                raise ValueError('catalogue: counterfactual k = %r outside 1 .. %d' % (k, MAX_K - 1))
            if side != 'item' or direction != 'down':
                raise ValueError("catalogue: counterfactual k goes with side='item' and direction='down' only, got side "
                                 "= %r, direction = %r: a user's review moves every item's score for that user, so the "
                                 "top-k list is not a fixed threshold" % (side, direction))
        if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)) \
                or not 1 <= budget <= ops.FOLD_SEARCH_MAX_BUDGET:
            raise ValueError('catalogue: counterfactual budget = %r outside 1 .. %d' % (budget, ops.FOLD_SEARCH_MAX_BUDGET))
        B = int(budget)
        u, i = self._pair_request(users, items)
        n = int(u.numel())
        if target is not None:
            if torch.is_tensor(target) or isinstance(target, (np.ndarray, list, tuple)):
                tgt = torch.as_tensor(target).detach().reshape(-1).to(torch.float32).cpu()
                if tgt.numel() != n:
                    raise ValueError('catalogue: counterfactual target holds %d values for %d pairs' % (tgt.numel(), n))
            elif isinstance(target, bool) or not isinstance(target, (int, float, np.integer, np.floating)):
                raise ValueError('catalogue: counterfactual target must be a float or one float per pair, got %r' % (target,))
            else:
                tgt = torch.full((n,), float(target), dtype=torch.float32)
        self._flush()
        i64 = lambda *s: torch.full(s, -1, dtype=torch.int64, device=self.dev)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)
        if n == 0:
            return Counterfactual(i64(0, B), i64(0, B), i64(0, B), f32(0, B + 1), i64(0), i64(0).to(torch.bool), f32(0), f32(0))
        tgt = self._leave_topk_targets(u, i, int(k)) if k is not None else tgt.to(self.dev)
        (pool_u, tower_u, _), (pool_i, tower_i, _) = self._phrase_side('user'), self._phrase_side('item')
        T = int(self.hp['input_length'])

        def live_bits(pool, ids):                              # the owner's first 64 reviews, one bit each
            count = np.minimum(pool.first[ids + 1] - pool.first[ids], WHATIF_MAX_SLOTS).astype(np.uint64)
            bits = np.where(count >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << np.minimum(count, np.uint64(63))) - np.uint64(1))
            return torch.from_numpy(bits.view(np.int64)).to(self.dev)
        with torch.no_grad():
            words = self._words().detach()
            ptab_u = ops.fold_project(words, tower_u.convs[0].weight.detach())
            ptab_i = ops.fold_project(words, tower_i.convs[0].weight.detach())
            order = torch.empty((n, B), dtype=torch.int32, device=self.dev)
            scores, steps, crossed = f32(n, B + 1), order.new_empty((n,)), order.new_empty((n,))
            step = max(1, int(self.pair_batch))
            for s0 in range(0, n, step):
                sl = slice(s0, s0 + step)
                uu, u_inv = np.unique(u[sl].numpy(), return_inverse=True)
                ui, i_inv = np.unique(i[sl].numpy(), return_inverse=True)
                dev = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int64)).to(self.dev)
                order[sl], scores[sl], steps[sl], crossed[sl] = ops.fold_search(
                    self._pair_kind, self._pair_head(u[sl].to(self.dev), i[sl].to(self.dev)),
                    self._fold_side(tower_u, pool_u, uu, ptab_u), self._fold_side(tower_i, pool_i, ui, ptab_i),
                    dev(u_inv), dev(i_inv), tgt[sl].contiguous(), 0 if direction == 'down' else 1, B, T,
                    cand_u=live_bits(pool_u, u[sl].numpy()) if side in ('user', 'both') else None,
                    cand_i=live_bits(pool_i, i[sl].numpy()) if side in ('item', 'both') else None)
            order = order.to(torch.int64)
            removed = _removed_by_side(order)
            return Counterfactual(removed[0], removed[1], order, scores, steps.to(torch.int64), crossed != 0,
                                  scores[:, 0].contiguous(), tgt)

    def deletion_curve(self, users, items, k=5, by='pair', side='user', direction='up'):
        """The ``k`` heaviest word windows of one side's document occluded CUMULATIVELY -> ``DocDeletionCurve`` of
        device tensors:

            scores     float32 [n, k + 1]  column 0 the prediction with nothing removed, column j the prediction with
                                           the first j windows of ``positions`` occluded; beyond ``live`` the last
                                           live column repeats
            aopc       float32 [n]         the mean over j = 1 .. live of scores[:, 0] - scores[:, j] (0 without a
                                           window): the area over the perturbation curve -- large when the windows
                                           named carry the score
            positions  int32 [n, k]        the windows' conv positions p in occlusion order, -1 unused: window p covers
                                           the document positions p - 2 .. p inside [0, input_length)
            live       int64 [n]           the number of windows the list really has

        ``by``: 'pair' -- ``explain_pair``'s windows of the side (this pair's gradient weights; ``direction`` as
        there); 'mass' -- ``explain_words`` without weights, the owner's heaviest windows whatever the pair; or an int
        tensor [n, k] of conv positions of your own in [0, input_length + 2), -1 (unused) only after the used ones.
        ``side``: 'user' or 'item'; the other side's document stays whole.  Refused before anything is enqueued: a bad
        ``by`` / ``side`` / ``direction`` / ``k`` (ValueError), unequal lengths (ValueError), an id outside its side's
        pool (KeyError), a configuration without a tower with the reason."""
        why = phrase_limits(self.hp)
        if why is not None:
            raise RuntimeError('reviews4rec_amd.recommend: ' + why)
        if side not in ('item', 'user'):
            raise ValueError("catalogue: side must be 'item' or 'user', got %r" % (side,))
        if direction not in ('up', 'down'):
            raise ValueError("catalogue: direction must be 'up' or 'down', got %r" % (direction,))
        T = int(self.hp['input_length'])
        F = int(self._phrase_side(side)[1].convs[0].bias.numel())
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= F:
            raise ValueError('catalogue: deletion_curve k = %r outside 1 .. %d' % (k, F))
        k = int(k)
        named = isinstance(by, str)
        if named and by not in ('pair', 'mass'):
            raise ValueError("catalogue: by must be 'pair', 'mass' or an int tensor [n, %d] of positions, got %r" % (k, by))
        u, i = self._whatif_request(users, items)
        n = len(u)
        if not named:
            pos = torch.as_tensor(by) if torch.is_tensor(by) or isinstance(by, (np.ndarray, list, tuple)) else None
            if pos is None or pos.dtype not in (torch.int32, torch.int64) or tuple(pos.shape) != (n, k):
                raise ValueError("catalogue: by must be 'pair', 'mass' or an int tensor [%d, %d] of positions, got %r"
                                 % (n, k, getattr(by, 'shape', by)))
            pos = pos.detach().cpu().to(torch.int64).numpy()
            used = pos >= 0
            if ((pos < -1) | (pos >= T + 2)).any() or (used[:, 1:] & ~used[:, :-1]).any():
                raise ValueError('catalogue: by as positions lies in [0, %d), with -1 (unused) only after the used ones'
                                 % (T + 2))
        elif n == 0:
            pos = np.zeros((0, k), np.int64)
        elif by == 'pair':
            pos = getattr(self.explain_pair(u, i, k=k, direction=direction), side).positions.cpu().numpy().astype(np.int64)
        else:
            pos = self.explain_words(u if side == 'user' else i, k=k, side=side).positions.cpu().numpy().astype(np.int64)
        used = pos >= 0
        live = used.sum(1)
        win = pos[:, :, None] - 2 + np.arange(3)[None, None, :]                   # [n, k, 3]: the words of window p
        win = np.where(used[:, :, None] & (win >= 0) & (win < T), win, -1).reshape(n, 1, 3 * k)
        upto = np.repeat(np.arange(k), 3)[None, None, :] <= np.arange(k)[None, :, None]
        occ = np.where(upto, win, -1)                                             # [n, k, 3 k]: variant j = windows 0 .. j
        ou, oi = (occ, None) if side == 'user' else (None, occ)
        scores, base, _ = self._what_if(u, i, None, None, ou, oi)
        live_d = torch.from_numpy(live).to(self.dev)
        col = torch.arange(k, device=self.dev)[None, :]
        last = torch.cat([base[:, None], scores], 1).gather(1, live_d[:, None])   # the last live column (the base: none)
        scores = torch.where(col < live_d[:, None], scores, last.expand(n, k))
        gain = (base[:, None].double() - scores.double()) * (col < live_d[:, None])
        aopc = (gain.sum(1) / live_d.clamp(min=1)).to(torch.float32)
        return DocDeletionCurve(torch.cat([base[:, None], scores], 1).contiguous(), aopc,
                                torch.from_numpy(pos.astype(np.int32)).to(self.dev), live_d)


def _removed_by_side(order):
    """A search's ``order`` int64 [n, B] (user slots, 64 + item slots, fill -1) -> [removed_user, removed_item], each
    side's steps moved to the front in step sequence, fill -1."""
    removed = []
    for lo in (0, ops.NARRE_SEARCH_ITEM):
        mine = (order >= lo) & (order < lo + ops.NARRE_SEARCH_ITEM)
        vals = torch.where(mine, order - lo, torch.full_like(order, -1))
        front = torch.sort((~mine).to(torch.int64), dim=1, stable=True).indices
        removed.append(vals.gather(1, front).contiguous())
    return removed


def _drop_masks(drop, count, what):
    """A ``drop`` argument of ``Catalogue.what_if`` -> int64 numpy masks [n, V] or None, checked against the owners'
    review counts ``count`` [n]."""
    n = len(count)
    if drop is None:
        return None
    if torch.is_tensor(drop) or isinstance(drop, np.ndarray):
        m = torch.as_tensor(drop)
        if m.dtype != torch.int64 or m.dim() != 2 or m.shape[0] != n or m.shape[1] < 1:
            raise ValueError('catalogue: %s as masks must be int64 [%d, V] with V >= 1, got %s %s'
                             % (what, n, m.dtype, tuple(m.shape)))
        return m.detach().cpu().contiguous().numpy()
    if not isinstance(drop, (list, tuple)) or len(drop) != n:
        raise ValueError('catalogue: %s must be None, int64 masks [n, V] or one list of review indices per pair (%d pairs)'
                         % (what, n))
    is_index = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    rows = []
    for p, entry in enumerate(drop):
        if not isinstance(entry, (list, tuple, np.ndarray)):
            raise ValueError('catalogue: %s[%d] must be a list of review indices (or a list of such lists)' % (what, p))
        entry = list(entry)
        variants = [entry] if all(is_index(v) for v in entry) else [list(v) if isinstance(v, (list, tuple, np.ndarray))
                                                                    else [v] for v in entry]
        row = []
        for variant in variants:
            mask = 0
            for v in variant:
                if not is_index(v) or not 0 <= int(v) < int(count[p]) or int(v) >= WHATIF_MAX_SLOTS:
                    raise ValueError('catalogue: %s[%d] names review %r outside the owner\'s list of %d (the first %d '
                                     'can be removed)' % (what, p, v, int(count[p]), WHATIF_MAX_SLOTS))
                mask |= 1 << int(v)
            row.append(mask - (1 << 64) if mask >= (1 << 63) else mask)
        rows.append(row)
    if n and any(len(row) != len(rows[0]) for row in rows):
        raise ValueError('catalogue: %s holds %s variants per pair; every pair needs as many'
                         % (what, sorted({len(row) for row in rows})))
    V = len(rows[0]) if n else 1
    if V < 1:
        raise ValueError('catalogue: %s holds no variant' % what)
    return np.array(rows, dtype=np.int64).reshape(n, V)


def _occlusions(occ, n, T, what):
    """An ``occlude`` argument of ``Catalogue.what_if`` -> int64 numpy [n, V, P] (-1 unused) or None; every position
    is -1 or inside [0, T)."""
    if occ is None:
        return None
    if torch.is_tensor(occ) or isinstance(occ, np.ndarray):
        a = torch.as_tensor(occ)
        if a.dtype not in (torch.int32, torch.int64) or a.dim() != 3 or a.shape[0] != n or a.shape[1] < 1:
            raise ValueError('catalogue: %s as a tensor must be int32 / int64 [%d, V, P] with V >= 1, got %s %s'
                             % (what, n, a.dtype, tuple(a.shape)))
        a = a.detach().cpu().to(torch.int64).contiguous().numpy()
    else:
        if not isinstance(occ, (list, tuple)) or len(occ) != n:
            raise ValueError('catalogue: %s must be None, an int tensor [n, V, P] or one list of positions per pair (%d '
                             'pairs)' % (what, n))
        is_index = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        rows = []
        for p, entry in enumerate(occ):
            if not isinstance(entry, (list, tuple, np.ndarray)):
                raise ValueError('catalogue: %s[%d] must be a list of positions (or a list of such lists)' % (what, p))
            entry = list(entry)
            variants = [entry] if all(is_index(v) for v in entry) else [list(v) if isinstance(v, (list, tuple, np.ndarray))
                                                                        else [v] for v in entry]
            if any(not is_index(v) for variant in variants for v in variant):
                raise ValueError('catalogue: %s[%d] holds something that is not a position' % (what, p))
            rows.append(variants)
        if n and any(len(row) != len(rows[0]) for row in rows):
            raise ValueError('catalogue: %s holds %s variants per pair; every pair needs as many'
                             % (what, sorted({len(row) for row in rows})))
        V = len(rows[0]) if n else 1
        if V < 1:
            raise ValueError('catalogue: %s holds no variant' % what)
        P = max([len(variant) for row in rows for variant in row] + [1])
        a = np.full((n, V, P), -1, np.int64)
        for p, row in enumerate(rows):
            for v, variant in enumerate(row):
                a[p, v, :len(variant)] = variant
    if ((a < -1) | (a >= T)).any():
        raise ValueError('catalogue: %s names a position outside [0, input_length = %d) (-1: unused)' % (what, T))
    return a


PairPhrases = namedtuple('PairPhrases', 'user item scores')      # Catalogue.explain_pair: two ``Phrases`` and [n] scores
PairReviews = namedtuple('PairReviews', 'w_user w_item rev_user rev_item glogit_user glogit_item attention_user '
                         'attention_item live_user live_item scores')          # NarreCatalogue.pair_reviews
WhatIf = namedtuple('WhatIf', 'scores base')                                    # NarreCatalogue.what_if
LeaveOneOut = namedtuple('LeaveOneOut', 'base without_user without_item delta_user delta_item live_user live_item')
DeletionCurve = namedtuple('DeletionCurve', 'scores aopc order live')           # NarreCatalogue.deletion_curve
Counterfactual = namedtuple('Counterfactual', 'removed_user removed_item order scores steps crossed base target')  # NarreCatalogue.counterfactual
Shapley = namedtuple('Shapley', 'phi_user phi_item base empty_user empty_item live_user live_item values')  # NarreCatalogue.shapley
DocLeaveOneOut = namedtuple('DocLeaveOneOut', LeaveOneOut._fields + ('reach_user', 'reach_item'))   # Catalogue.leave_one_out
DocDeletionCurve = namedtuple('DocDeletionCurve', 'scores aopc positions live')                    # Catalogue.deletion_curve
WHATIF_MAX_SLOTS = 64               # r4r_narre_whatif, r4r_tower_build_variants: one bit of an int64 mask per slot
PHRASE_FILTERS = 100                # every TextCNN tower's filter count (common_pytorch_models.py:11)
_PHRASE_TYPES = ('deepconn', 'deepconn++', 'transnet', 'transnet++', 'NARRE')
Phrases = namedtuple('Phrases', 'positions scores filters tokens reviews offsets windows slots weights',
                     defaults=(None, None))        # Catalogue.explain_words; slots / weights: NarreCatalogue's


def phrase_limits(hyper_params):
    """None when this configuration has a TextCNN tower whose windows ``explain_words`` can list, else the reason."""
    mt = hyper_params['model_type']
    if mt not in _PHRASE_TYPES:
        return ('model_type %r has no TextCNN tower (its two sides are id embeddings): there are no word windows to '
                'explain' % (mt,))
    return None


RELU_MAX_L = 128                   # r4r_topk_relu: H <= 128, P <= 128
_NEUMF_STAGES = ('GMF', 'MLP', 'NeuMF')


def relu_catalogue_limits(hyper_params):
    """None when ``ReluCatalogue`` can rank this configuration, else the reason it cannot."""
    mt = hyper_params['model_type']
    served = _served_before(mt, 1)
    if served:
        return served
    if mt not in ('deepconn++', 'NeuMF'):
        why = _REFUSED.get(mt)
        return 'model_type %r has no ReLU-sum form%s' % (mt, ': ' + why if why else '')
    if mt == 'NeuMF' and hyper_params.get('neumf_stage', 'NeuMF') not in _NEUMF_STAGES:
        return 'neumf_stage %r is none of %r' % (hyper_params.get('neumf_stage'), _NEUMF_STAGES)
    if _latent_size(hyper_params) > RELU_MAX_L:
        return 'latent_size %d > %d' % (_latent_size(hyper_params), RELU_MAX_L)
    return None


def _relu_kind(hyper_params):
    mt = hyper_params['model_type']
    return 'deepconn++' if mt == 'deepconn++' else hyper_params.get('neumf_stage', 'NeuMF')


def fold_relu_head(params, hyper_params, side, x=None, gx=None, bias=None, dtype=torch.float32):
    """One side of a Linear -> ReLU -> linear head over [user | item] as the rows of the ReLU-sum (include/r4r.h):

        score(u, i) = sum_{j<H} w_j relu(qa[u][j] + ca[i][j]) + sum_{j<P} qp[u][j] cp[i][j] + q_bias[u] + c_bias[i]

        kind        H  P  qa[u]               ca[i]           w         qp[u] / cp[i]                    q_bias[u]
        deepconn++  L  0  W0[:, :L] zu + b0   W0[:, L:] zi    final.3.weight[0]   -                      ub + g + final.3.bias
        MLP         L  0  W1[:, :L] ue + b1   W1[:, L:] ie    f W3      -                                ub + g + final.bias + f . b3
        NeuMF       L  L  as MLP (mlp_* tables, f = final.weight[0, L:])  gmf_ue * final.weight[0, :L] / gmf_ie   as MLP
        GMF         0  L  -                   -               -         ue * final.weight[0] / ie        ub + g + final.bias

    (W0 = final.0.weight; W1, b1, W3, b3 = project.1 / project.3; c_bias[i] is item_bias[i]; dropout is the identity in
    eval mode.)  ``params``: the model's parameters by state_dict key; the kind is hyper_params' model_type and, for
    NeuMF, neumf_stage.  ``x`` [n, L]: the side's tower latents (deepconn++) or MLP embedding rows; ``gx`` [n, L]: its
    GMF embedding rows (GMF: the only table); ``bias`` [n]: its rows of user_bias / item_bias.
    -> side 'user': (rows [n, H + P], q_bias [n], w [H]);  side 'item': (rows [n, H + P], c_bias [n]).
    Plain torch on whatever device the inputs live on, computed in float64 and rounded once to ``dtype``."""
    if side not in ('user', 'item'):
        raise ValueError("fold_relu_head: side must be 'user' or 'item', got %r" % (side,))
    kind = _relu_kind(hyper_params)
    if kind not in ('deepconn++',) + _NEUMF_STAGES:
        raise ValueError('fold_relu_head: no ReLU-sum form for %r' % (kind,))
    f64 = lambda t: t.detach().to(torch.float64)
    need_x, need_g = kind != 'GMF', kind in ('GMF', 'NeuMF')
    if (x is None) == need_x or (gx is None) == need_g or bias is None:
        raise ValueError('fold_relu_head: %s takes %s' % (kind, ' and '.join(
            n for n, on in (('x', need_x), ('gx', need_g), ('bias', True)) if on)))
    ref = x if need_x else gx
    if ref.dim() != 2 or bias.dim() != 1 or bias.shape[0] != ref.shape[0] or (need_x and need_g and gx.shape != x.shape):
        raise ValueError('fold_relu_head: x / gx [n, L] and bias [n] do not match')
    n, L = ref.shape
    user = side == 'user'
    b = f64(bias)
    if user:
        b = b + f64(params['global_bias']).reshape(())
    parts, w = [], torch.zeros(0, dtype=torch.float64, device=ref.device)
    if need_x:
        if kind == 'deepconn++':
            W, b_in, out_w, out_b = (params[k] for k in ('final.0.weight', 'final.0.bias', 'final.3.weight', 'final.3.bias'))
            if tuple(W.shape) != (L, 2 * L) or out_w.numel() != L:
                raise ValueError('fold_relu_head: final.0.weight %s / final.3.weight %s do not match latent width %d'
                                 % (tuple(W.shape), tuple(out_w.shape), L))
            w, extra = f64(out_w).reshape(-1), f64(out_b).reshape(())
        else:
            W, b_in, W3, b3, fin, fin_b = (params[k] for k in ('project.1.weight', 'project.1.bias', 'project.3.weight',
                                                               'project.3.bias', 'final.weight', 'final.bias'))
            width = 2 * L if kind == 'NeuMF' else L
            if tuple(W.shape) != (L, 2 * L) or tuple(W3.shape) != (L, L) or tuple(fin.shape) != (1, width):
                raise ValueError('fold_relu_head: project / final %s %s %s do not match latent width %d'
                                 % (tuple(W.shape), tuple(W3.shape), tuple(fin.shape), L))
            f = f64(fin)[0, width - L:]
            w, extra = f @ f64(W3), f64(fin_b).reshape(()) + f @ f64(b3)
        Ws = f64(W)[:, :L] if user else f64(W)[:, L:]
        a = f64(x) @ Ws.T
        if user:
            a, b = a + f64(b_in), b + extra
        parts.append(a)
    if need_g:
        fin = params['final.weight']
        if tuple(fin.shape) != (1, 2 * L if kind == 'NeuMF' else L):
            raise ValueError('fold_relu_head: final.weight %s does not match latent width %d' % (tuple(fin.shape), L))
        g = f64(gx)
        if user:
            g = g * f64(fin)[0, :L]
            if kind == 'GMF':
                b = b + f64(params['final.bias']).reshape(())
        parts.append(g)
    rows = torch.cat(parts, 1) if len(parts) > 1 else parts[0]
    return (rows.to(dtype), b.to(dtype), w.to(dtype)) if user else (rows.to(dtype), b.to(dtype))


class ReluCatalogue(Catalogue):
    """``Catalogue``'s surface (``refresh``, ``recommend``, ``score_pairs``, ``rank``; the same return types, devices,
    (-1, -inf) fill and argument checks: the three calls are ``Catalogue``'s own, over this class's ``_head``) for the
    ReLU-sum families: deepconn++ and the three NeuMF stages (``fold_relu_head``), ranked by r4r_topk_relu /
    r4r_pair_relu / r4r_rank_relu.

    ``refresh()`` flushes the engine's pending table updates and caches the item side (``c``, ``c_bias`` with -inf in
    ineligible rows, ``w``): deepconn++ runs the item documents through the tower ``tower_batch`` at a time, NeuMF
    takes the embedding tables through one small matmul.  The query side is computed per call from the current
    weights.  A pass leaves the training state untouched.  No CPU and no torch fallback.  ``main``'s hooks reach this
    class for deepconn++ only; NeuMF is served here and through ``eval_catalogue(catalogue=ReluCatalogue(...))``."""

    _form = 'relu'
    _limits = staticmethod(relu_catalogue_limits)

    def _shape(self):
        self.kind = _relu_kind(self.hp)
        L = _latent_size(self.hp)
        self.H, self.P = {'deepconn++': (L, 0), 'MLP': (L, 0), 'NeuMF': (L, L), 'GMF': (0, L)}[self.kind]
        self.D = self.H + self.P
        # one row per item id (deepconn++), or the item tables as they are (total_items + 1)
        self.n_c = self.n_items if self.kind == 'deepconn++' else int(self.model.item_bias.numel())

    def _tables(self, side):
        m = self.model
        if self.kind == 'NeuMF':
            return getattr(m, 'mlp_%s_embedding' % side).weight.detach(), getattr(m, 'gmf_%s_embedding' % side).weight.detach()
        t = getattr(m, '%s_embedding' % side).weight.detach()
        return (None, t) if self.kind == 'GMF' else (t, None)

    def refresh(self):
        self._flush()
        m, P = self.model, self._params()
        elig, mask, ninf = self._eligible_rows()
        with torch.no_grad():
            if self.kind != 'deepconn++':
                x, gx = self._tables('item')
                c, cb = fold_relu_head(P, self.hp, 'item', x=x, gx=gx, bias=m.item_bias.detach())
                self.c, self.c_bias = c.contiguous(), torch.where(mask, cb, ninf)
            else:
                c = torch.zeros((self.n_c, self.D), dtype=torch.float32, device=self.dev)
                for sl, _, z in self._latents(m.item_conv, self.reader.store.items, self.eligible):
                    sel = elig[sl]
                    c[sel], ninf[sel] = fold_relu_head(P, self.hp, 'item', x=z, bias=m.item_bias.detach()[sel])
                self.c, self.c_bias = c, ninf
            # w is the user side's; the fold of zero user rows yields it without a tower forward
            L = _latent_size(self.hp)
            none = torch.zeros((0, L), dtype=torch.float32, device=self.dev)
            self.w = fold_relu_head(P, self.hp, 'user', x=none if self.kind != 'GMF' else None,
                                    gx=none if self.kind in ('GMF', 'NeuMF') else None, bias=none[:, 0])[2].contiguous()
            if self.w.numel() == 0:
                self.w = torch.zeros(1, dtype=torch.float32, device=self.dev)          # (H = 0: never read, never null)

    def _queries(self, u_host):
        """(q [n, H + P], q_bias [n]) of the requested users from the current weights."""
        m, P = self.model, self._params()
        u = u_host.to(self.dev)
        with torch.no_grad():
            ub = m.user_bias.detach()[u]
            if self.kind != 'deepconn++':
                x, gx = self._tables('user')
                q, qb, _ = fold_relu_head(P, self.hp, 'user', x=None if x is None else x[u], gx=None if gx is None else gx[u],
                                          bias=ub)
                return q.contiguous(), qb.contiguous()
            q = torch.empty((u.numel(), self.D), dtype=torch.float32, device=self.dev)
            qb = torch.empty((u.numel(),), dtype=torch.float32, device=self.dev)
            for sl, _, z in self._latents(m.user_conv, self.reader.store.users, u_host.numpy()):
                q[sl], qb[sl], _ = fold_relu_head(P, self.hp, 'user', x=z, bias=ub[sl])
            return q, qb

    def _head(self, q, n, qb):
        return (ptr(q), n, ptr(qb), ptr(self.c), self.n_c, self.D, ptr(self.c_bias), ptr(self.w), self.H, self.P)

    _pair_kind = 'mlp'

    def _pair_head(self, u, i):
        """deepconn++ (DeepCoNN.py:68-72): final.0 / final.3 as they are; q_bias = user_bias + global_bias +
        final.3.bias, c_bias = item_bias.  (NeuMF has no tower: ``_pair_limits`` refuses it before this is reached.)"""
        m, P = self.model, self._params()
        f64 = lambda t: t.detach().to(torch.float64)
        qb = f64(m.user_bias)[u] + f64(P['global_bias']).reshape(()) + f64(P['final.3.bias']).reshape(())
        return dict(W0=P['final.0.weight'], b0=P['final.0.bias'], w3=P['final.3.weight'].reshape(-1),
                    q_bias=qb.to(torch.float32).contiguous(), c_bias=m.item_bias.detach()[i].contiguous())


HMLP_MAX_L = 64                     # r4r_topk_hmlp: D <= 64, H <= 64
NARRE_ATTN_MAX = 32                 # r4r_narre_attn_fwd: R <= 32, L <= 32; beyond, r4r_narre_explain (R, L <= 64)
Explanation = namedtuple('Explanation', 'slots reviews reviewers weights attention live')   # NarreCatalogue.explain


def narre_catalogue_limits(hyper_params):
    """None when ``NarreCatalogue`` can rank this configuration, else the reason it cannot."""
    from .data import NEIGHBOURS
    mt = hyper_params['model_type']
    served = _served_before(mt, 2)
    if served:
        return served
    if mt != 'NARRE':
        why = _REFUSED.get(mt)
        return 'model_type %r has no product-MLP form%s' % (mt, ': ' + why if why else '')
    if _latent_size(hyper_params) > HMLP_MAX_L:
        return 'latent_size %d > %d' % (_latent_size(hyper_params), HMLP_MAX_L)
    R = int(hyper_params.get('narre_num_reviews', NEIGHBOURS))
    if R != NEIGHBOURS:
        return ('narre_num_reviews %d is not the width of the neighbour lists, %d (NARRE.py:56 concatenates the two)'
                % (R, NEIGHBOURS))
    return None


class NarreCatalogue(Catalogue):
    """``Catalogue``'s surface (``refresh``, ``recommend``, ``score_pairs``, ``rank``; the same return types, devices,
    (-1, -inf) fill and argument checks: the three calls are ``Catalogue``'s own, over this class's ``_head``) for NARRE,
    ranked by r4r_topk_hmlp / r4r_pair_hmlp / r4r_rank_hmlp.

    NARRE's attention weighs the reviews of one side by the id embeddings of THAT side's neighbours -- the items a
    user's own reviews are about, the users who reviewed an item (NARRE.py:110-113) -- and a rating outside the training
    split removes nothing from either list (data.py:240-246).  So

        au[u] = attention_user(zu[u, 0..R), item_embedding[reviewed_items[u]]) + user_embedding[u]        per user
        ai[i] = attention_item(zi[i, 0..R), user_embedding[users_who_reviewed[i]]) + item_embedding[i]    per item, cached
        score(u, i) = final.3(relu(final.1(au[u] * ai[i]))) + user_bias[u] + item_bias[i] + global_bias

    ``refresh()`` flushes the engine's pending row updates and caches the item side (``c`` = ai, ``c_bias`` = item_bias
    with -inf in ineligible rows, ``W``, ``b``, ``w`` from final.1 / final.3), ``tower_batch`` items at a time: one tower
    forward per review and the eval-mode attention.  The query side is computed per call from the current weights.  A
    pass leaves the training state untouched.  No CPU and no torch fallback.  ``main``'s ``recommend_k`` /
    ``catalogue_metrics_k`` hooks do not reach this class; NARRE is served here and through
    ``eval_catalogue(catalogue=NarreCatalogue(...))``.

    The attention runs through r4r_narre_attn_fwd where that takes the shape (R and L up to 32) and through
    r4r_narre_explain (csrc/narre_explain.hip: R and L up to 64) beyond.  ``explain`` returns what the attention says:
    each owner's most useful reviews (``main``'s ``explain_k`` hook writes them for every eligible item).
    ``pair_reviews`` says how much each review carries ONE pair's score, to first order; ``what_if`` /
    ``leave_one_out`` / ``deletion_curve`` say what the score would be with reviews removed, exactly and in the
    loader's own sense of removed (csrc/narre_whatif.hip)."""

    _form = 'hmlp'
    _limits = staticmethod(narre_catalogue_limits)

    def _shape(self):
        self.D = self.H = _latent_size(self.hp)
        self.n_c = self.n_items                                # one row per item id

    def _attended(self, side, ids, **how):
        """au (side 'user') or ai ('item') [n, L] of the owners ``ids`` (a host int64 array) from the current weights:
        every review of the owner and its neighbour ids with nothing removed (data.py:240-246; pad id total + 1 of
        the OTHER side, data.py:275-276), one eval-mode tower forward per review, the eval-mode attention, the owner's
        id embedding.  ``how``: ``_attend``'s ``explain_k``."""
        from .data import _np_neighbours, _np_reviews
        hp = self.hp
        user, pool, conv, pad = self._narre_side(side)
        ids = np.asarray(ids, dtype=np.int64)
        if len(ids) and (ids.min() < 0 or ids.max() >= pool.owners):
            raise KeyError('id outside the review pools: {}'.format(int(ids.max())))
        R, Wd = int(hp['narre_num_reviews']), int(hp['narre_num_words'])
        rb, re = pool.first[ids], pool.first[ids + 1]
        none = np.full(len(ids), -1, np.int64)
        reviews = _np_reviews(pool.tok, pool.rev_off, rb, re, none, R, Wd)
        nb = torch.from_numpy(_np_neighbours(pool.nb, rb, re, none, pad)).to(self.dev)
        with torch.no_grad():
            z = self._tower(conv, torch.from_numpy(reviews.reshape(len(ids) * R, Wd)).to(self.dev)).view(len(ids), R, -1)
            return self._attend(side, z, nb, ids, **how)

    def _narre_side(self, side):
        """(user, pool, tower, pad id of the neighbour lists: total + 1 of the OTHER side) of 'user' / 'item'."""
        user, m = side == 'user', self.model
        return ((True, self.reader.store.users, m.user_conv, self.n_items + 1) if user else
                (False, self.reader.store.items, m.item_conv, self.n_users + 1))

    def _attend(self, side, z, nb, ids, explain_k=None, jac=False):
        """The eval-mode attention over review latents ``z`` [n, R, L] weighed by the neighbours ``nb`` [n, 10], plus
        the id embedding of the owners ``ids`` (a host int64 array).  Where r4r_narre_attn_fwd takes the shape (R and L
        up to 32) it is that call, as before; beyond, r4r_narre_explain's ``out`` with the owners' rows added in the
        kernel.  ``explain_k``: no pooled vector but ``explain``'s pieces of these owners, from r4r_narre_explain at
        every L -> (attention [n, R], top_slot int32 [n, k], top_w [n, k], live int32 [n], nb).  ``jac``: the owner pass
        of ``pair_reviews``, r4r_narre_attn_jac at every L -> a dict with p, z, attn, E, dz (``ops.narre_pair_grad``'s
        side) and live int64 [n]."""
        m, user = self.model, side == 'user'
        scorer = m.attention_scorer_user if user else m.attention_scorer_item
        own, other = (m.user_embedding, m.item_embedding) if user else (m.item_embedding, m.user_embedding)
        weights = (scorer[0].weight.detach(), scorer[0].bias.detach(), scorer[3].weight.detach(), scorer[3].bias.detach())
        ids = np.asarray(ids, dtype=np.int64)
        with torch.no_grad():
            if jac:
                _, pool, tower, _ = self._narre_side(side)
                got = ops.narre_attn_jac(z, nb, other.weight.detach(), *weights, fc=tower.fc.weight.detach(),
                                         own_table=own.weight.detach(), owner=torch.from_numpy(ids).to(self.dev),
                                         want=('attn', 'out', 'E', 'dz'))
                live = np.minimum(pool.first[ids + 1] - pool.first[ids], z.shape[1]).astype(np.int64)
                return dict(p=got['out'], z=z, attn=got['attn'], E=got['E'], dz=got['dz'],
                            live=torch.from_numpy(live).to(self.dev))
            if explain_k is not None:
                first = self._narre_side(side)[1].first
                live = torch.from_numpy(np.minimum(first[ids + 1] - first[ids], z.shape[1]).astype(np.int32)).to(self.dev)
                _, attn, top_slot, top_w = ops.narre_explain(z, nb, other.weight.detach(), *weights, live=live,
                                                             k=explain_k, want_out=False)
                return attn, top_slot, top_w, live, nb
            owners = torch.from_numpy(ids).to(self.dev)
            if z.shape[1] > NARRE_ATTN_MAX or z.shape[2] > NARRE_ATTN_MAX:
                return ops.narre_explain(z, nb, other.weight.detach(), *weights, own_table=own.weight.detach(),
                                         owner=owners, want_attn=False)[0]
            att = ops.narre_attention(z, other.weight.detach()[nb].contiguous(), *weights, 0.0, False, None)
            return att + own.weight.detach()[owners]

    def _attended_chunks(self, side, ids, **how):
        """(sl, ``_attended(side, ids[sl])``) over the ``tower_batch`` chunks of ``ids`` (a host int64 array); with
        towers 'device' the review latents and the neighbour ids are slices of one r4r_tower_span_fwd pass."""
        if self.towers != 'device' or len(ids) == 0:
            for sl, chunk in self._batches(ids):
                yield sl, self._attended(side, chunk, **how)
            return
        _, pool, conv, pad = self._narre_side(side)
        R = int(self.hp['narre_num_reviews'])
        z, nb = self._span_latents(conv, pool, ids, narre_pad=pad)
        z = z.view(len(ids), R, -1)
        for sl, chunk in self._batches(ids):
            yield sl, self._attend(side, z[sl], nb[sl], chunk, **how)

    def explain(self, ids, k=3, side='item'):
        """The reviews that carry an owner's attended vector: per item (``side='item'``; 'user': per user, among the
        user's own reviews) the ``k`` heaviest REAL reviews by NARRE's attention (NARRE.py:53-64, eval mode, from the
        current weights) -> ``Explanation`` of device tensors, n = len(ids):

            slots      int64 [n, k]    the review's slot among the owner's first R reviews; fill -1
            reviews    int64 [n, k]    its index in that side's pool, ``pool.first[id] + slot`` (``pool.rev_off`` /
                                       ``pool.tok`` give its tokens); fill -1
            reviewers  int64 [n, k]    the slot's neighbour id: the user who wrote the review ('item'), the item it is
                                       about ('user'); fill -1
            weights    float32 [n, k]  the slots' attention weights, descending, ties by ascending slot; fill 0
            attention  float32 [n, R]  the model's weights of every slot, padded slots included: rows sum to 1
            live       int64 [n]       min(number of reviews, R): only an owner's first R reviews take part
                                       (data.py:144-172)

        The weights are the model's own: the softmax runs over all R slots, padded ones included (the reference does
        not mask them), and nothing is renormalised over the live slots -- a padded slot is never LISTED, but the
        listed weights of an owner with fewer than R reviews sum to less than 1.  One r4r_narre_explain call per
        ``tower_batch`` chunk at every latent size, for both ``towers`` modes.  ``ids``: a list, an array or a tensor
        on any device; an id outside the side's pool raises KeyError, ``k`` outside 1..R and a ``side`` other than
        'item' / 'user' raise ValueError.  The engine's pending updates are flushed first, as ``refresh()`` does; the
        training state is left untouched."""
        if side not in ('item', 'user'):
            raise ValueError("catalogue: side must be 'item' or 'user', got %r" % (side,))
        R = int(self.hp['narre_num_reviews'])
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= R:
            raise ValueError('catalogue: explain k = %r outside 1 .. %d' % (k, R))
        k = int(k)
        ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1).cpu().numpy()
        pool = self.reader.store.users if side == 'user' else self.reader.store.items
        if len(ids) and (ids.min() < 0 or ids.max() >= pool.owners):
            raise KeyError('id outside the review pools: {}'.format(int(ids.max())))
        self._flush()
        n = len(ids)
        slots = torch.full((n, k), -1, dtype=torch.int64, device=self.dev)
        weights = torch.zeros((n, k), dtype=torch.float32, device=self.dev)
        attention = torch.empty((n, R), dtype=torch.float32, device=self.dev)
        live = torch.zeros((n,), dtype=torch.int64, device=self.dev)
        reviewers = torch.full((n, k), -1, dtype=torch.int64, device=self.dev)
        for sl, (attn, top_slot, top_w, lv, nb) in self._attended_chunks(side, ids, explain_k=k):
            s = top_slot.to(torch.int64)
            slots[sl], weights[sl], attention[sl], live[sl] = s, top_w, attn, lv
            reviewers[sl] = torch.where(s >= 0, nb.gather(1, s.clamp(min=0)), s)
        first = torch.from_numpy(pool.first[ids]).to(self.dev)
        reviews = torch.where(slots >= 0, first[:, None] + slots, slots)
        return Explanation(slots, reviews, reviewers, weights, attention, live)

    def _phrase_side(self, side):
        _, pool, tower, pad = self._narre_side(side)
        return pool, tower, pad

    def _pair_limits(self):
        return ("model_type 'NARRE' has no pair explanation: its review latents reach the score through the softmax "
                "of the review attention (NARRE.py:53-64), and a gradient through it is not built")

    # ------------------------------------------------------------------ pair explanations per REVIEW
    pair_batch = 8192      # pairs per r4r_narre_pair_grad call of ``pair_reviews``; set after construction

    def _pair_reviews(self, u, i):
        """``pair_reviews`` of checked host id tensors."""
        self._flush()
        m = self.model
        R = int(self.hp['narre_num_reviews'])
        n = int(u.numel())
        F = int(m.user_conv.fc.weight.shape[1])
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)
        i64 = lambda *s: torch.empty(s, dtype=torch.int64, device=self.dev)
        out = PairReviews(f32(n, R, F), f32(n, R, F), f32(n, R), f32(n, R), f32(n, R), f32(n, R), f32(n, R), f32(n, R),
                          i64(n), i64(n), f32(n))
        if n == 0:
            return out
        uu, u_inv = torch.unique(u, return_inverse=True)
        ui, i_inv = torch.unique(i, return_inverse=True)
        with torch.no_grad():
            sides = []
            for side, ids in (('user', uu), ('item', ui)):
                parts = [part for _, part in self._attended_chunks(side, ids.numpy(), jac=True)]
                s = {key: torch.cat([part[key] for part in parts]).contiguous() for key in parts[0]}
                s['fc'] = self._narre_side(side)[2].fc.weight.detach()
                sides.append(s)
            su, si = sides
            f64 = lambda t: t.detach().to(torch.float64)
            qb = (f64(m.user_bias).reshape(-1)[uu.to(self.dev)] + f64(m.global_bias).reshape(())
                  + f64(m.final[3].bias).reshape(())).to(torch.float32).contiguous()
            cb = m.item_bias.detach().reshape(-1)[ui.to(self.dev)].to(torch.float32).contiguous()
            W1, b1, w = m.final[1].weight.detach(), m.final[1].bias.detach(), m.final[3].weight.detach().reshape(-1)
            u_inv, i_inv = u_inv.to(self.dev), i_inv.to(self.dev)
            step = max(1, int(self.pair_batch))
            for s0 in range(0, n, step):
                sl = slice(s0, s0 + step)
                got = ops.narre_pair_grad(su, si, u_inv[sl].contiguous(), i_inv[sl].contiguous(), W1, b1, w, q_bias=qb,
                                          c_bias=cb, want=('score', 'glogit_user', 'glogit_item', 'rev_user', 'rev_item',
                                                           'w_user', 'w_item'))
                out.w_user[sl], out.w_item[sl] = got['w_user'], got['w_item']
                out.rev_user[sl], out.rev_item[sl] = got['rev_user'], got['rev_item']
                out.glogit_user[sl], out.glogit_item[sl] = got['glogit_user'], got['glogit_item']
                out.scores[sl] = got['score']
            out.attention_user.copy_(su['attn'][u_inv])
            out.attention_item.copy_(si['attn'][i_inv])
            out.live_user.copy_(su['live'][u_inv])
            out.live_item.copy_(si['live'][i_inv])
        return out

    def pair_reviews(self, users, items):
        """Why THIS item for THIS user, per REVIEW: for the pairs (users[p], items[p]) (lists, arrays or tensors on any
        device, equally long; owners of the review pools) -> ``PairReviews`` of device tensors, n = len(users):

            w_user, w_item                  float32 [n, R, F]  d score / d pooled[r, f] of the side's tower for slot r,
                                            through the attention's softmax: what ``explain_words(..., weights=)`` takes
            rev_user, rev_item              float32 [n, R]     gradient . input of slot r's latent: how much review r
                                            carries THIS pair's score (a_r g . z_r + delta_r D_r . z_r)
            glogit_user, glogit_item        float32 [n, R]     d score / d logit_r of the attention; rows sum to 0
            attention_user, attention_item  float32 [n, R]     ``explain``'s ``attention`` of the pair's owners, bit for bit
            live_user, live_item            int64 [n]          ``explain``'s ``live``
            scores                          float32 [n]        the model's eval-mode prediction, from the raw head parameters

        The DISTINCT users and items go once through the towers (both ``towers`` modes: the same bits) and the owner
        pass r4r_narre_attn_jac; the pairs go through r4r_narre_pair_grad, ``pair_batch`` at a time (the results do not
        depend on it) -- include/r4r.h, "NARRE pair gradients".  The score's scalars (user bias, global bias,
        final.3.bias) are summed in float64 and rounded once.  Unequal lengths raise ValueError, an id outside its side's
        pool KeyError, before anything is enqueued.  The engine's pending updates are flushed first, as ``refresh()``
        does; the training state is left untouched."""
        return self._pair_reviews(*self._pair_request(users, items))

    def explain_pair_reviews(self, users, items, k=5, reviews=None, direction='up'):
        """The reviews and the words behind one user-item score -> ``PairPhrases(user, item, scores)``: ``user`` is
        ``explain_words(users, k, 'user', weights=+-w_user)`` and ``item`` is ``explain_words(items, k, 'item',
        weights=+-w_item)`` of ``pair_reviews(users, items)``, bit for bit (they are made by those calls): [n, R, k] per
        side.  ``direction``: 'up' lists what RAISES the prediction most (+w, +rev), 'down' what lowers it most.
        ``reviews=k_r``: the lists are cut to the ``k_r`` LIVE slots with the largest +-rev (ties by ascending slot):
        [n, k_r, k], with ``slots`` [n, k_r] holding those slots and ``weights`` [n, k_r] their ``rev`` values; a place
        beyond the owner's live slots holds ``explain_words``' fill (slot -1, weight 0).  Refused before anything is
        enqueued, in this order: a ``direction`` other than 'up' / 'down', ``k`` outside 1 .. F, ``reviews`` outside
        1 .. R, unequal lengths (ValueError), an id outside its side's pool (KeyError)."""
        if direction not in ('up', 'down'):
            raise ValueError("catalogue: direction must be 'up' or 'down', got %r" % (direction,))
        R = int(self.hp['narre_num_reviews'])
        F = int(self._phrase_side('item')[1].convs[0].bias.numel())
        if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= F:
            raise ValueError('catalogue: explain_pair_reviews k = %r outside 1 .. %d' % (k, F))
        if reviews is not None and (isinstance(reviews, bool) or not isinstance(reviews, (int, np.integer))
                                    or not 1 <= reviews <= R):
            raise ValueError('catalogue: explain_pair_reviews reviews = %r outside 1 .. %d' % (reviews, R))
        u, i = self._pair_request(users, items)
        pr = self._pair_reviews(u, i)
        sign = 1.0 if direction == 'up' else -1.0
        sides = []
        for ids, side, w, rev, live in ((u, 'user', pr.w_user, pr.rev_user, pr.live_user),
                                        (i, 'item', pr.w_item, pr.rev_item, pr.live_item)):
            ph = self.explain_words(ids, k=int(k), side=side, weights=w if direction == 'up' else -w)
            if reviews is not None:
                ph = self._cut_to_reviews(ph, sign * rev, rev, live, int(reviews))
            sides.append(ph)
        return PairPhrases(sides[0], sides[1], pr.scores)

    def _cut_to_reviews(self, ph, key, rev, live, k_r):
        """``ph`` ([n, R, ...]) cut to the ``k_r`` live slots with the largest ``key`` [n, R], ties by ascending slot."""
        n, R = key.shape
        slot_of = torch.arange(R, device=self.dev)[None, :]
        key = torch.where(slot_of < live[:, None], key, torch.full_like(key, float('-inf')))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :k_r]
        none = torch.arange(k_r, device=self.dev)[None, :] >= live[:, None]
        slots = order.masked_fill(none, -1)
        take = order

        def pick(t, fill):
            tail = (1,) * (t.dim() - 2)
            rows = t.gather(1, take.view(take.shape + tail).expand(take.shape + t.shape[2:]))
            return rows.masked_fill(none.view(none.shape + tail), fill).contiguous()
        return Phrases(pick(ph.positions, -1), pick(ph.scores, 0), pick(ph.filters, 0), pick(ph.tokens, -1),
                       pick(ph.reviews, -1), pick(ph.offsets, -1), pick(ph.windows, 0), slots, pick(rev, 0))

    # ------------------------------------------------------------------ what-if scores: a pair's rating with reviews removed
    def _whatif_drops(self, drop, ids, side, what):
        """One side's ``drop`` argument of ``what_if`` -> (int64 host masks [n, V] or None, the most drops of any
        variant); everything is checked here, before anything is enqueued."""
        n = int(ids.numel())
        if drop is None:
            return None, 0
        if torch.is_tensor(drop) or isinstance(drop, np.ndarray):
            m = torch.as_tensor(drop)
            if m.dtype != torch.int64 or m.dim() != 2 or m.shape[0] != n or m.shape[1] < 1:
                raise ValueError('catalogue: %s as masks must be int64 [%d, V] with V >= 1, got %s %s'
                                 % (what, n, m.dtype, tuple(m.shape)))
            m = m.detach().cpu().contiguous()
            bits = np.unpackbits(m.numpy().view(np.uint8).reshape(n, -1, 8), axis=-1).sum(-1) if n else np.zeros((0, 1))
            return m, int(bits.max()) if bits.size else 0
        if not isinstance(drop, (list, tuple)) or len(drop) != n:
            raise ValueError('catalogue: %s must be None, int64 masks [n, V] or one list of review indices per pair (%d pairs)'
                             % (what, n))
        pool = self._narre_side(side)[1]
        count = pool.first[ids.numpy() + 1] - pool.first[ids.numpy()]
        is_index = lambda v: isinstance(v, (int, np.integer)) and not isinstance(v, bool)
        rows, most = [], 0
        for p, entry in enumerate(drop):
            if not isinstance(entry, (list, tuple, np.ndarray)):
                raise ValueError('catalogue: %s[%d] must be a list of review indices (or a list of such lists)' % (what, p))
            entry = list(entry)
            variants = [entry] if all(is_index(v) for v in entry) else [list(v) if isinstance(v, (list, tuple, np.ndarray))
                                                                        else [v] for v in entry]
            row = []
            for variant in variants:
                mask = 0
                for v in variant:
                    if not is_index(v) or not 0 <= int(v) < int(count[p]) or int(v) >= WHATIF_MAX_SLOTS:
                        raise ValueError('catalogue: %s[%d] names review %r outside the owner\'s list of %d (the first %d '
                                         'can be removed)' % (what, p, v, int(count[p]), WHATIF_MAX_SLOTS))
                    mask |= 1 << int(v)
                most = max(most, bin(mask).count('1'))
                row.append(mask - (1 << 64) if mask >= (1 << 63) else mask)
            rows.append(row)
        if n and any(len(row) != len(rows[0]) for row in rows):
            raise ValueError('catalogue: %s holds %s variants per pair; every pair needs as many'
                             % (what, sorted({len(row) for row in rows})))
        V = len(rows[0]) if n else 1
        if V < 1:
            raise ValueError('catalogue: %s holds no variant' % what)
        return torch.tensor(rows, dtype=torch.int64).reshape(n, V), most

    def _whatif_side(self, side, ids, S):
        """``ops.narre_whatif``'s side for the owners ``ids`` (a host int64 array) over S >= R slots: the latents and
        neighbour ids of the first R reviews as ``_attended`` builds them, those of the reviews R .. S - 1 R at a time
        the same way -- ``data._np_review_slots`` and the tower per chunk ('host'), one shifted r4r_tower_span_fwd pass
        ('device'): the same bits -- the logits of all S slots from
        r4r_narre_logits, and the padding slot: the tower on an all-padding review with the pad id's logit."""
        from .data import _np_neighbours, _np_review_slots, _np_reviews
        m, hp = self.model, self.hp
        user, pool, conv, pad = self._narre_side(side)
        R, Wd = int(hp['narre_num_reviews']), int(hp['narre_num_words'])
        scorer = m.attention_scorer_user if user else m.attention_scorer_item
        own, other = (m.user_embedding, m.item_embedding) if user else (m.item_embedding, m.user_embedding)
        weights = (scorer[0].weight.detach(), scorer[0].bias.detach(), scorer[3].weight.detach(), scorer[3].bias.detach())
        ids = np.asarray(ids, dtype=np.int64)
        n = len(ids)
        docs_of = lambda d: torch.from_numpy(np.ascontiguousarray(d).reshape(-1, Wd)).to(self.dev)
        with torch.no_grad():
            if self.towers == 'device':
                z, nb = self._span_latents(conv, pool, ids, narre_pad=pad)
                z = z.view(n, R, -1)
            else:
                zs, nbs = [], []
                for _, chunk in self._batches(ids):
                    rb, re = pool.first[chunk], pool.first[chunk + 1]
                    none = np.full(len(chunk), -1, np.int64)
                    zs.append(self._tower(conv, docs_of(_np_reviews(pool.tok, pool.rev_off, rb, re, none, R, Wd))).view(len(chunk), R, -1))
                    nbs.append(torch.from_numpy(_np_neighbours(pool.nb, rb, re, none, pad)).to(self.dev))
                z, nb = torch.cat(zs), torch.cat(nbs)
            for lo in range(R, S, R):                          # the slots that can slide in, R at a time: the same towers
                if self.towers == 'device':
                    zb, nbb = self._span_latents(conv, pool, ids, narre_pad=pad, shift=lo)
                    zb = zb.view(n, R, -1)
                else:
                    zs, nbs = [], []
                    for _, chunk in self._batches(ids):
                        docs, neigh = _np_review_slots(pool.tok, pool.rev_off, pool.nb, pool.first[chunk],
                                                       pool.first[chunk + 1], lo, lo + R, Wd, pad)
                        zs.append(self._tower(conv, docs_of(docs)).view(len(chunk), R, -1))
                        nbs.append(torch.from_numpy(neigh).to(self.dev))
                    zb, nbb = torch.cat(zs), torch.cat(nbs)
                z, nb = torch.cat([z, zb], 1), torch.cat([nb, nbb], 1)
            z, nb = z[:, :S].contiguous(), nb[:, :S].contiguous()
            z_pad = self._tower(conv, torch.zeros((1, Wd), dtype=torch.int64, device=self.dev)).reshape(-1)
            table = other.weight.detach()
            logit = ops.narre_logits(z, nb, table, *weights)
            pad_id = torch.full((1, 1), int(pad), dtype=torch.int64, device=self.dev)
            logit_pad = float(ops.narre_logits(z_pad.view(1, 1, -1), pad_id, table, *weights).reshape(()))
            live = np.minimum(pool.first[ids + 1] - pool.first[ids], R).astype(np.int64)
            return dict(z=z, logit=logit, own=own.weight.detach()[torch.from_numpy(ids).to(self.dev)].contiguous(),
                        z_pad=z_pad, logit_pad=logit_pad, R=R, live=torch.from_numpy(live).to(self.dev))

    def _what_if(self, u, i, mask_u, mask_i, most_u, most_i, slide):
        """``what_if`` of checked host tensors -> (scores [n, V], base [n], live_user [n], live_item [n]); the pairs'
        own prediction rides along as one more variant (nothing removed)."""
        self._flush()
        m = self.model
        R = int(self.hp['narre_num_reviews'])
        n = int(u.numel())
        V = next((int(t.shape[1]) for t in (mask_u, mask_i) if t is not None), 1)
        if n == 0:
            e = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=self.dev)
            return e(0, V), e(0), e(0, dt=torch.int64), e(0, dt=torch.int64)
        drops = []
        for t in (mask_u, mask_i):
            d = torch.zeros((n, V + 1), dtype=torch.int64)
            if t is not None:
                d[:, 1:] = t
            drops.append(d.to(self.dev))
        uu, u_inv = torch.unique(u, return_inverse=True)
        ui, i_inv = torch.unique(i, return_inverse=True)
        slots = lambda most: min(WHATIF_MAX_SLOTS, R + most) if slide else R
        with torch.no_grad():
            su = self._whatif_side('user', uu.numpy(), slots(most_u))
            si = self._whatif_side('item', ui.numpy(), slots(most_i))
            f64 = lambda t: t.detach().to(torch.float64)
            qb = (f64(m.user_bias).reshape(-1)[uu.to(self.dev)] + f64(m.global_bias).reshape(())
                  + f64(m.final[3].bias).reshape(())).to(torch.float32).contiguous()
            cb = m.item_bias.detach().reshape(-1)[ui.to(self.dev)].to(torch.float32).contiguous()
            W1, b1, w = m.final[1].weight.detach(), m.final[1].bias.detach(), m.final[3].weight.detach().reshape(-1)
            u_inv, i_inv = u_inv.to(self.dev), i_inv.to(self.dev)
            out = torch.empty((n, V + 1), dtype=torch.float32, device=self.dev)
            step = max(1, int(self.pair_batch))
            for s0 in range(0, n, step):
                sl = slice(s0, s0 + step)
                out[sl] = ops.narre_whatif(su, si, u_inv[sl].contiguous(), i_inv[sl].contiguous(), drops[0][sl].contiguous(),
                                           drops[1][sl].contiguous(), W1, b1, w, q_bias=qb, c_bias=cb)
            return out[:, 1:].contiguous(), out[:, 0].contiguous(), su['live'][u_inv], si['live'][i_inv]

    def what_if(self, users, items, drop_user=None, drop_item=None, slide=True):
        """What would the model predict for (users[p], items[p]) if chosen reviews were not there?  -> ``WhatIf(scores
        [n, V], base [n])`` of device tensors: ``scores[p, v]`` is the eval-mode prediction with variant v's reviews
        removed from the user's and / or the item's list, ``base[p]`` the prediction with nothing removed.

        ``drop_user`` / ``drop_item``: None (nothing removed on that side); or, per pair, a list of review indices in
        the owner's pool order -- the loader's ``skip`` (data.py:144-172) -- as one variant, or a list of such lists as
        V variants (every pair as many); or an int64 mask tensor [n, V], bit s = the owner's review s removed.  Both
        sides given: the same V.  ``slide=True`` is the loader's removal: slot r holds the r-th REMAINING review, the
        owner's reviews beyond R slide in (each side reaches S = min(64, R + the most drops of any variant) reviews of
        its owners), padding fills the tail -- exactly what a training rating sees of its own pair.  ``slide=False`` is
        occlusion: S = R, the removed reviews' places go to padding at the tail.

        No tower runs per variant: a review enters NARRE's score through its latent and its attention logit alone
        (NARRE.py:53-64).  The DISTINCT users and items go once through the towers (both ``towers`` modes: the same
        bits) and the owner pass r4r_narre_logits; the pairs go through r4r_narre_whatif, ``pair_batch`` at a time (the
        results do not depend on it) -- include/r4r.h, "NARRE what-if scores".  The score's scalars are summed in
        float64 and rounded once, as ``pair_reviews`` does.  Before anything is enqueued: unequal lengths, a malformed
        drop, unequal V and a review index outside the owner's list (or beyond the first 64) raise ValueError, an id
        outside its side's pool KeyError.  The engine's pending updates are flushed first; the training state is left
        untouched."""
        u, i = self._pair_request(users, items)
        mask_u, most_u = self._whatif_drops(drop_user, u, 'user', 'drop_user')
        mask_i, most_i = self._whatif_drops(drop_item, i, 'item', 'drop_item')
        if mask_u is not None and mask_i is not None and mask_u.shape[1] != mask_i.shape[1]:
            raise ValueError('catalogue: drop_user holds %d variants per pair, drop_item %d'
                             % (mask_u.shape[1], mask_i.shape[1]))
        scores, base, _, _ = self._what_if(u, i, mask_u, mask_i, most_u, most_i, bool(slide))
        return WhatIf(scores, base)

    def leave_one_out(self, users, items, slide=True):
        """Each attended review of each pair removed in turn -> ``LeaveOneOut`` of device tensors, n = len(users):

            base                          float32 [n]     the prediction with nothing removed
            without_user, without_item    float32 [n, R]  the prediction without the owner's review in slot r
            delta_user, delta_item        float32 [n, R]  base - without: what review r adds to THIS pair's score
            live_user, live_item          int64 [n]       ``explain``'s ``live``: min(number of reviews, R)

        A slot at or beyond ``live`` holds no review: ``without`` is ``base`` there and ``delta`` exactly 0.  ``slide``:
        as ``what_if`` (True: the owner's review R + 1 moves up, the loader's ``skip``).  One ``what_if`` pass of 2 R
        variants per pair; its checks and refusals."""
        u, i = self._pair_request(users, items)
        R, n = int(self.hp['narre_num_reviews']), int(u.numel())
        one = (torch.ones(R, dtype=torch.int64) << torch.arange(R, dtype=torch.int64))[None, :].expand(n, R)
        none = torch.zeros((n, R), dtype=torch.int64)
        scores, base, live_u, live_i = self._what_if(u, i, torch.cat([one, none], 1), torch.cat([none, one], 1), 1, 1,
                                                     bool(slide))
        slot = torch.arange(R, device=self.dev)[None, :]
        held = base[:, None].expand(n, R)
        without_u = torch.where(slot < live_u[:, None], scores[:, :R], held).contiguous()
        without_i = torch.where(slot < live_i[:, None], scores[:, R:], held).contiguous()
        return LeaveOneOut(base, without_u, without_i, held - without_u, held - without_i, live_u, live_i)

    def deletion_curve(self, users, items, by='rev', side='user', direction='up', slide=True):
        """The live reviews of one side removed CUMULATIVELY, the largest key first -> ``DeletionCurve`` of device tensors:

            scores  float32 [n, R + 1]  column 0 the prediction with nothing removed (``what_if``'s ``base``), column k
                                        the prediction with the first k reviews of ``order`` removed; beyond the
                                        owner's live reviews the last live column repeats
            aopc    float32 [n]         the mean over k = 1 .. live of scores[:, 0] - scores[:, k] (0 with no review):
                                        the area over the perturbation curve -- large when the key names the reviews
                                        that carry the score
            order   int64 [n, R]        the slots in removal order; -1 beyond ``live``
            live    int64 [n]           min(number of reviews, R)

        ``by``: 'rev' -- ``pair_reviews``' gradient x input of the side; 'attention' -- ``explain``'s weights;
        'shapley' -- ``shapley``'s ``phi`` of the side's one-side game, with the same ``slide``; or a float tensor
        [n, R] of your own.  ``direction`` 'up' removes the largest key first, 'down' the smallest; ties go
        to the ascending slot.  ``side``: 'user' or 'item'; the other side keeps every review.  ``slide``: as
        ``what_if``.  Refused before anything is enqueued: a bad ``by`` / ``side`` / ``direction`` (ValueError), unequal
        lengths (ValueError), an id outside its side's pool (KeyError)."""
        if side not in ('item', 'user'):
            raise ValueError("catalogue: side must be 'item' or 'user', got %r" % (side,))
        if direction not in ('up', 'down'):
            raise ValueError("catalogue: direction must be 'up' or 'down', got %r" % (direction,))
        R = int(self.hp['narre_num_reviews'])
        named = isinstance(by, str)
        if named and by not in ('rev', 'attention', 'shapley'):
            raise ValueError("catalogue: by must be 'rev', 'attention', 'shapley' or a tensor [n, %d], got %r" % (R, by))
        u, i = self._pair_request(users, items)
        n = int(u.numel())
        if not named:
            if not (torch.is_tensor(by) or isinstance(by, np.ndarray)) or tuple(by.shape) != (n, R) \
                    or not torch.as_tensor(by).dtype.is_floating_point:
                raise ValueError("catalogue: by must be 'rev', 'attention' or a float tensor [%d, %d], got %r"
                                 % (n, R, getattr(by, 'shape', by)))
            key = torch.as_tensor(by).detach().to(self.dev, torch.float32)
        ids = u if side == 'user' else i
        pool = self._narre_side(side)[1]
        count = pool.first[ids.numpy() + 1] - pool.first[ids.numpy()]
        live = torch.from_numpy(np.minimum(count, R).astype(np.int64)).to(self.dev)
        if named and n and by == 'rev':
            key = getattr(self._pair_reviews(u, i), 'rev_' + side)
        elif named and by == 'shapley':                        # the side's one-side game, with the same slide
            key = getattr(self.shapley(u, i, side=side, slide=slide), 'phi_' + side)
        elif named and n:                                      # the DISTINCT owners' attention, handed to their pairs
            distinct, inverse = torch.unique(ids, return_inverse=True)
            key = self.explain(distinct, k=1, side=side).attention[inverse.to(self.dev)]
        elif named:
            key = torch.empty((0, R), dtype=torch.float32, device=self.dev)
        if direction == 'down':
            key = -key
        slot = torch.arange(R, device=self.dev)[None, :]
        valid = slot < live[:, None]
        key = torch.where(valid, key, torch.full_like(key, float('-inf')))
        order = torch.sort(key, dim=1, descending=True, stable=True).indices
        bit = torch.where(valid, torch.ones_like(order) << order, torch.zeros_like(order))
        masks = torch.cumsum(bit, dim=1).cpu()                  # distinct bits: the sum is the union
        mu, mi = (masks, None) if side == 'user' else (None, masks)
        most = (R, 0) if side == 'user' else (0, R)
        scores, base, _, _ = self._what_if(u, i, mu, mi, most[0], most[1], bool(slide))
        gain = (base[:, None].double() - scores.double()) * valid
        aopc = (gain.sum(1) / live.clamp(min=1)).to(torch.float32)
        return DeletionCurve(torch.cat([base[:, None], scores], 1).contiguous(), aopc,
                             torch.where(valid, order, torch.full_like(order, -1)), live)

    # ------------------------------------------------------------------ counterfactuals: the fewest reviews that flip a score
    def review_counterfactual(self, *args, **kw):
        """Refused: NARRE reads its reviews one by one and a removal re-selects slots; its search is ``counterfactual``."""
        raise RuntimeError('reviews4rec_amd.recommend: review_counterfactual folds the one document of a deepconn / '
                           'deepconn++ / transnet tower; NARRE reads its reviews one by one: use '
                           'NarreCatalogue.counterfactual')

    def counterfactual(self, users, items, target=None, k=None, direction='down', side='both', budget=None, slide=True):
        """Which reviews would have to be missing for the model to stop predicting ``target`` for (users[p], items[p]),
        and how few are enough?  A greedy search, whole on the device: at each step every review the model currently
        attends on the chosen side(s) is removed in turn (the loader's removal, as ``what_if``), the removal that moves
        the score furthest in ``direction`` is kept -- even when it moves the score the wrong way -- and the search
        ends when the score has passed the target, after ``budget`` removals, or when no attended review is left
        -> ``Counterfactual`` of device tensors, n = len(users), B = ``budget``:

            removed_user, removed_item  int64 [n, B]    the side's removed reviews as indices in the owner's pool order
                                                        (what ``what_if`` takes), in step sequence; fill -1
            order    int64 [n, B]        the step's number c: the review's slot for a user review, 64 + the slot for an
                                         item review; -1 beyond the last step
            scores   float32 [n, B + 1]  column 0 the prediction with nothing removed, column t the prediction after
                                         step t; beyond the last step the last score repeats
            steps    int64 [n]           the removals made
            crossed  bool [n]            the last score passed the target (strictly)
            base     float32 [n]         scores[:, 0]: ``what_if``'s ``base``
            target   float32 [n]         the threshold each pair was held to

        Exactly one of ``target`` and ``k``.  ``target``: a float or one float per pair, a rating threshold; the pair is
        done when score < target (``direction='down'``) or score > target ('up').  ``k``: "the item leaves this
        user's top-k": the target is the score of the k-th best eligible unseen OTHER item from ``recommend(users,
        k + 1)`` (-inf where the user has fewer than k other items: such a pair never crosses).  ``k`` goes with
        ``side='item'`` and ``direction='down'`` only: a user's review moves EVERY item's score for that user, so with
        a user side the list is not a fixed threshold.  The threshold is in ``recommend``'s bits while the search
        compares r4r_narre_whatif's bits (the two differ as ``what_if``'s ``base`` differs from ``score_pairs``), and an
        exact tie counts as not crossed.

        ``side``: 'user', 'item' or 'both' -- the candidates are the owner's live reviews of that side or sides.
        ``budget``: 1 .. 64, default the side's R (R_u + R_i for 'both', capped at 64).  ``slide=True``: each searched
        side reaches S = min(64, R + budget) reviews of its owners, so that every removal has its slide-in
        (``what_if``'s slot path, both ``towers`` modes); ``slide=False``: S = R, occlusion.  The greedy answer is an
        upper bound of the fewest removals, not the minimum.

        The DISTINCT owners go once through the towers and r4r_narre_logits; the pairs go ``pair_batch`` at a time
        through r4r_narre_search (include/r4r.h, "NARRE counterfactual search"; the results do not depend on the
        batch).  Every score is ``what_if``'s score of the same removals, bit for bit.  Before anything is enqueued: a
        ``side`` / ``direction`` outside the above, both or neither of ``target`` / ``k``, ``k`` outside 1 .. 127 or
        with a user side or 'up', ``budget`` outside 1 .. 64, unequal lengths and a ``target`` tensor of another length
        raise ValueError, an id outside its side's pool KeyError.  The engine's pending updates are flushed first; the
        training state is left untouched."""
        if side not in ('user', 'item', 'both'):
            raise ValueError("catalogue: side must be 'user', 'item' or 'both', got %r" % (side,))
        if direction not in ('up', 'down'):
            raise ValueError("catalogue: direction must be 'up' or 'down', got %r" % (direction,))
        if (target is None) == (k is None):
            raise ValueError('catalogue: counterfactual takes exactly one of target and k, got target = %r and k = %r'
                             % (target, k))
        if k is not None:
            if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= MAX_K - 1:
                raise ValueError('catalogue: counterfactual k = %r outside 1 .. %d' % (k, MAX_K - 1))
            if side != 'item' or direction != 'down':
                raise ValueError("catalogue: counterfactual k goes with side='item' and direction='down' only, got side "
                                 "= %r, direction = %r: a user's review moves every item's score for that user, so the "
                                 "top-k list is not a fixed threshold" % (side, direction))
        R = int(self.hp['narre_num_reviews'])
        if budget is None:
            budget = min(ops.NARRE_SEARCH_MAX_BUDGET, 2 * R if side == 'both' else R)
        if isinstance(budget, bool) or not isinstance(budget, (int, np.integer)) \
                or not 1 <= budget <= ops.NARRE_SEARCH_MAX_BUDGET:
            raise ValueError('catalogue: counterfactual budget = %r outside 1 .. %d' % (budget, ops.NARRE_SEARCH_MAX_BUDGET))
        B = int(budget)
        u, i = self._pair_request(users, items)
        n = int(u.numel())
        if target is not None:
            if torch.is_tensor(target) or isinstance(target, (np.ndarray, list, tuple)):
                tgt = torch.as_tensor(target).detach().reshape(-1).to(torch.float32).cpu()
                if tgt.numel() != n:
                    raise ValueError('catalogue: counterfactual target holds %d values for %d pairs' % (tgt.numel(), n))
            elif isinstance(target, bool) or not isinstance(target, (int, float, np.integer, np.floating)):
                raise ValueError('catalogue: counterfactual target must be a float or one float per pair, got %r' % (target,))
            else:
                tgt = torch.full((n,), float(target), dtype=torch.float32)
        self._flush()
        m = self.model
        i64 = lambda *s: torch.full(s, -1, dtype=torch.int64, device=self.dev)
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)
        if n == 0:
            return Counterfactual(i64(0, B), i64(0, B), i64(0, B), f32(0, B + 1), i64(0), i64(0).to(torch.bool), f32(0), f32(0))
        tgt = self._leave_topk_targets(u, i, int(k)) if k is not None else tgt.to(self.dev)
        on_u, on_i = side in ('user', 'both'), side in ('item', 'both')
        slots = lambda on: min(WHATIF_MAX_SLOTS, R + B) if (slide and on) else R
        uu, u_inv = torch.unique(u, return_inverse=True)
        ui, i_inv = torch.unique(i, return_inverse=True)

        def live_mask(which, ids, inv, S):                     # the owner's reviews among the S slots, one bit each:
            pool = self._narre_side(which)[1]                  # once per DISTINCT owner, handed to the owner's pairs
            count = np.minimum(pool.first[ids.numpy() + 1] - pool.first[ids.numpy()], S).astype(np.uint64)
            bits = np.where(count >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << np.minimum(count, np.uint64(63))) - np.uint64(1))
            return torch.from_numpy(bits.view(np.int64)).to(self.dev)[inv]
        with torch.no_grad():
            su = self._whatif_side('user', uu.numpy(), slots(on_u))
            si = self._whatif_side('item', ui.numpy(), slots(on_i))
            cand_u = live_mask('user', uu, u_inv.to(self.dev), slots(on_u)) if on_u else None
            cand_i = live_mask('item', ui, i_inv.to(self.dev), slots(on_i)) if on_i else None
            f64 = lambda t: t.detach().to(torch.float64)
            qb = (f64(m.user_bias).reshape(-1)[uu.to(self.dev)] + f64(m.global_bias).reshape(())
                  + f64(m.final[3].bias).reshape(())).to(torch.float32).contiguous()
            cb = m.item_bias.detach().reshape(-1)[ui.to(self.dev)].to(torch.float32).contiguous()
            W1, b1, w = m.final[1].weight.detach(), m.final[1].bias.detach(), m.final[3].weight.detach().reshape(-1)
            u_inv, i_inv = u_inv.to(self.dev), i_inv.to(self.dev)
            order = torch.empty((n, B), dtype=torch.int32, device=self.dev)
            scores, steps, crossed = f32(n, B + 1), order.new_empty((n,)), order.new_empty((n,))
            step = max(1, int(self.pair_batch))
            for s0 in range(0, n, step):
                sl = slice(s0, s0 + step)
                part = lambda t: None if t is None else t[sl].contiguous()
                order[sl], scores[sl], steps[sl], crossed[sl] = ops.narre_search(
                    su, si, part(u_inv), part(i_inv), W1, b1, w, part(tgt), 0 if direction == 'down' else 1, B,
                    cand_u=part(cand_u), cand_i=part(cand_i), q_bias=qb, c_bias=cb)
            order = order.to(torch.int64)
            removed = _removed_by_side(order)
            return Counterfactual(removed[0], removed[1], order, scores, steps.to(torch.int64), crossed != 0,
                                  scores[:, 0].contiguous(), tgt)

    # ------------------------------------------------------------------ attributions: exact Shapley values of the reviews
    def shapley(self, users, items, side='both', joint=False, slide=True, values=False):
        """How much of the prediction for (users[p], items[p]) does each attended review carry?  The exact Shapley value
        of the game "which of these reviews are present": the one share-out that is efficient (the shares add up to
        what the reviews carry together), symmetric and exact -- ``leave_one_out`` double-counts redundant reviews and
        misses those that matter only once another is gone -> ``Shapley`` of device tensors, n = len(users):

            phi_user, phi_item      float32 [n, R]  review r's share of THIS pair's score; exactly 0 at a slot that holds
                                                    no review and on a side that does not play
            base                    float32 [n]     the prediction with nothing removed (``what_if``'s ``base``)
            empty_user, empty_item  float32 [n]     the prediction with every player of that side's game removed:
                                                    sum(phi_user) = base - empty_user up to the rounding (``base`` on a
                                                    side that does not play; with ``joint`` both hold the score with
                                                    both sides' reviews removed)
            live_user, live_item    int64 [n]       ``explain``'s ``live``: min(number of reviews, R)
            values                  None, or with ``values=True`` (user game's table, item game's table): float32
                                                    [n, 2^P] each (None for a side that does not play; with ``joint``
                                                    the one table twice), P the most players of any pair: entry c of
                                                    row p is the prediction with exactly the players whose bit in c is
                                                    set PRESENT (player t: the game's t-th live review, the user's
                                                    first in a joint game); entries from 2^(the pair's players) on are
                                                    not written

        The players are the pair's live reviews among the first R slots: the reviews the model attends with nothing
        removed.  ``side``: 'user' / 'item' plays one game with the other side intact; 'both' plays the two one-side
        games.  ``joint=True`` plays ONE game over both sides' reviews (``side`` must be 'both').  A game takes at most
        16 players: more on any pair is refused.  ``slide=True`` is the loader's removal -- each played side reaches
        S = min(64, R + its players) reviews of its owners, as ``what_if`` does; ``slide=False`` is occlusion, S = R.

        The DISTINCT owners go once through the towers and r4r_narre_logits; the pairs go ``pair_batch`` at a time
        through r4r_narre_shapley (include/r4r.h, "NARRE Shapley values"; the results do not depend on the batch).
        Every coalition's score is ``what_if``'s score of the same removals, bit for bit.  The score's scalars are summed
        in float64 and rounded once.  Before anything is enqueued: a bad ``side``, ``joint`` with one side, unequal
        lengths and a game of more than 16 players raise ValueError, an id outside its side's pool KeyError.  The
        engine's pending updates are flushed first; the training state is left untouched."""
        if side not in ('user', 'item', 'both'):
            raise ValueError("catalogue: side must be 'user', 'item' or 'both', got %r" % (side,))
        if joint and side != 'both':
            raise ValueError("catalogue: shapley joint=True plays one game over both sides: side must be 'both', got %r"
                             % (side,))
        R = int(self.hp['narre_num_reviews'])
        u, i = self._pair_request(users, items)
        n = int(u.numel())
        on_u, on_i = side in ('user', 'both'), side in ('item', 'both')
        uu, u_inv = torch.unique(u, return_inverse=True)
        ui, i_inv = torch.unique(i, return_inverse=True)

        def live_of(which, ids):                               # min(number of reviews, R) of the DISTINCT owners
            pool = self._narre_side(which)[1]
            return np.minimum(pool.first[ids.numpy() + 1] - pool.first[ids.numpy()], R).astype(np.int64)
        live_u, live_i = live_of('user', uu), live_of('item', ui)
        most_u = int(live_u.max()) if (n and on_u) else 0
        most_i = int(live_i.max()) if (n and on_i) else 0
        most = int((live_u[u_inv.numpy()] + live_i[i_inv.numpy()]).max()) if (n and joint) else max(most_u, most_i)
        if most > ops.NARRE_SHAPLEY_MAX_PLAYERS:
            raise ValueError('catalogue: shapley takes at most %d players a game; the largest of this request has %d%s'
                             % (ops.NARRE_SHAPLEY_MAX_PLAYERS, most, ' (joint=True counts both sides)' if joint else ''))
        self._flush()
        m = self.model
        f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)
        if n == 0:
            i64 = torch.empty((0,), dtype=torch.int64, device=self.dev)
            table = lambda on: f32(0, 2) if on else None
            return Shapley(f32(0, R), f32(0, R), f32(0), f32(0), f32(0), i64, i64.clone(),
                           (table(on_u), table(on_i)) if values else None)
        slots = lambda players: min(WHATIF_MAX_SLOTS, R + players) if slide else R
        bits = lambda live, inv: torch.from_numpy((np.int64(1) << live) - 1).to(self.dev)[inv]
        with torch.no_grad():
            su = self._whatif_side('user', uu.numpy(), slots(most_u))
            si = self._whatif_side('item', ui.numpy(), slots(most_i))
            f64 = lambda t: t.detach().to(torch.float64)
            qb = (f64(m.user_bias).reshape(-1)[uu.to(self.dev)] + f64(m.global_bias).reshape(())
                  + f64(m.final[3].bias).reshape(())).to(torch.float32).contiguous()
            cb = m.item_bias.detach().reshape(-1)[ui.to(self.dev)].to(torch.float32).contiguous()
            W1, b1, w = m.final[1].weight.detach(), m.final[1].bias.detach(), m.final[3].weight.detach().reshape(-1)
            u_inv, i_inv = u_inv.to(self.dev), i_inv.to(self.dev)
            play_u, play_i = bits(live_u, u_inv), bits(live_i, i_inv)
            # the games: (the user side's players, the item side's, the most players of a pair)
            games = ([(play_u, play_i, most)] if joint else
                     ([(play_u, None, most_u)] if on_u else []) + ([(None, play_i, most_i)] if on_i else []))
            zero = torch.zeros((n, R), dtype=torch.float32, device=self.dev)
            phi = [zero, zero.clone()]
            base, empty, tables = f32(n), [None, None], [None, None]
            step = max(1, int(self.pair_batch))
            for pu, pi, players in games:
                P = max(players, 1)
                g_phi = [f32(n, R) if pl is not None else None for pl in (pu, pi)]
                g_empty, g_table = f32(n), f32(n, 1 << P) if values else None
                for s0 in range(0, n, step):
                    sl = slice(s0, s0 + step)
                    part = lambda t: None if t is None else t[sl].contiguous()
                    got = ops.narre_shapley(su, si, part(u_inv), part(i_inv), W1, b1, w, play_u=part(pu), play_i=part(pi),
                                            P=P, q_bias=qb, c_bias=cb, values=values)
                    for k in (0, 1):
                        if g_phi[k] is not None:
                            g_phi[k][sl] = got[k][:, :R]
                    base[sl], g_empty[sl] = got[2], got[3]
                    if values:
                        g_table[sl] = got[5]
                for k, pl in enumerate((pu, pi)):
                    if pl is not None:
                        phi[k], empty[k], tables[k] = g_phi[k], g_empty, g_table
            empty = [base if e is None else e for e in empty]
            return Shapley(phi[0], phi[1], base, empty[0], empty[1], su['live'][u_inv], si['live'][i_inv],
                           tuple(tables) if values else None)

    def explain_words(self, ids, k=5, side='item', weights=None, reviews=None):
        """``Catalogue.explain_words`` per REVIEW: NARRE's towers read an owner's first R reviews one by one
        (NARRE.py:95-96), so there is one list of windows per (owner, slot) -> ``Phrases`` with [n, R, k] (tokens
        [n, R, k, 3], windows [n, R]); ``reviews=k_r``: [n, k_r, k], the phrases of the ``k_r`` reviews ``explain``
        lists, in its order, with its ``slots`` [n, k_r] and ``weights`` [n, k_r] alongside (a slot of -1 -- an owner
        with fewer than k_r reviews -- holds the fill: positions -1, scores 0, filters 0, tokens -1, windows 0).

            reviews    int64  ``pool.first[id] + slot`` where the slot holds a review and the window's first in-review
                              word lies inside it, else -1
            offsets    int64  that word's offset inside the review, max(p - 2, 0); -1 with reviews == -1

        ``weights``: as ``Catalogue.explain_words``; a tensor [n, F] weighs every review of owner n alike, a tensor
        [n, R, F] holds one row per review (``pair_reviews``' ``w_user`` / ``w_item``)."""
        R = int(self.hp['narre_num_reviews'])
        if reviews is not None and (isinstance(reviews, bool) or not isinstance(reviews, (int, np.integer))
                                    or not 1 <= reviews <= R):
            raise ValueError('catalogue: explain_words reviews = %r outside 1 .. %d' % (reviews, R))
        ids, pool, tower, pad, wt = self._phrase_request(ids, k, side, weights, per=R)
        k, n, W = int(k), len(ids), int(self.hp['narre_num_words'])
        self._flush()
        with torch.no_grad():
            pos, score, filt, tokens, win = self._phrase_rows(tower, pool, ids, k, wt, narre_pad=pad)
        pos, score, filt, tokens, win = (pos.view(n, R, k), score.view(n, R, k), filt.view(n, R, k),
                                         tokens.view(n, R, k, 3), win.view(n, R))
        slot = torch.arange(R, dtype=torch.int64, device=self.dev)[None, :].expand(n, R)
        listed = None
        if reviews is not None:
            e = self.explain(ids, k=int(reviews), side=side)
            listed, slot = e, e.slots
            take, none = slot.clamp(min=0), slot < 0

            def pick(t, fill):                                 # the rows of the listed slots; the fill where none is
                tail = (1,) * (t.dim() - 2)
                rows = t.gather(1, take.view(take.shape + tail).expand(take.shape + t.shape[2:]))
                return rows.masked_fill(none.view(none.shape + tail), fill)
            pos, score, filt, tokens, win = pick(pos, -1), pick(score, 0), pick(filt, 0), pick(tokens, -1), pick(win, 0)
        _, rev_off, first, _ = pool.device(self.dev)
        own = torch.from_numpy(ids).to(self.dev)
        rev = first[own][:, None] + slot                                           # the slot's review in the pool
        held = (slot >= 0) & (rev < first[own + 1][:, None])
        rev = torch.where(held, rev, torch.zeros_like(rev)).clamp(max=max(rev_off.numel() - 2, 0))
        length = (rev_off[(rev + 1).clamp(max=rev_off.numel() - 1)] - rev_off[rev]).clamp(max=W)
        t0 = (pos.to(torch.int64) - 2).clamp(min=0)
        inside = (pos >= 0) & held[:, :, None] & (t0 < length[:, :, None])
        minus = torch.full_like(t0, -1)
        out_rev = torch.where(inside, rev[:, :, None].expand_as(t0), minus)
        out_off = torch.where(inside, t0, minus)
        return Phrases(pos.contiguous(), score.contiguous(), filt.contiguous(), tokens.contiguous(), out_rev, out_off,
                       win.contiguous(), None if listed is None else listed.slots, None if listed is None else listed.weights)

    def refresh(self):
        self._flush()
        m = self.model
        elig, _, cb = self._eligible_rows()
        c = torch.zeros((self.n_c, self.D), dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            for sl, a in self._attended_chunks('item', self.eligible):
                c[elig[sl]] = a
            cb[elig] = m.item_bias.detach()[elig]
            self.c, self.c_bias = c, cb
            self.W = m.final[1].weight.detach().to(torch.float32).contiguous().clone()
            self.b = m.final[1].bias.detach().to(torch.float32).contiguous().clone()
            self.w = m.final[3].weight.detach().to(torch.float32).reshape(-1).contiguous().clone()

    def _queries(self, u_host):
        """(q [n, L], q_bias [n]) of the requested users from the current weights."""
        m = self.model
        u = u_host.to(self.dev)
        q = torch.empty((u.numel(), self.D), dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            for sl, a in self._attended_chunks('user', u_host.numpy()):
                q[sl] = a
            qb = (m.user_bias.detach()[u] + m.global_bias.detach()) + m.final[3].bias.detach().reshape(())
        return q, qb.contiguous()

    def _head(self, q, n, qb):
        return (ptr(q), n, ptr(qb), ptr(self.c), self.n_c, self.D, ptr(self.c_bias), ptr(self.W), ptr(self.b), ptr(self.w),
                self.D, self.H)


RFM_MAX_L = 64                      # r4r_topk_rfm: H <= 64, P <= 16, M <= 80
_TRANSNET_EMB = 5                   # the width of transnet++'s id embeddings (TransNet.py:75-76)


def transnet_catalogue_limits(hyper_params):
    """None when ``TransNetCatalogue`` can rank this configuration, else the reason it cannot."""
    mt = hyper_params['model_type']
    served = _served_before(mt, 3)
    if served:
        return served
    if mt not in ('transnet', 'transnet++'):
        why = _REFUSED.get(mt)
        return 'model_type %r has no ReLU-FM form: no class serves it%s' % (mt, ' (' + why + ')' if why else '')
    if _latent_size(hyper_params) > RFM_MAX_L:
        return 'latent_size %d > %d' % (_latent_size(hyper_params), RFM_MAX_L)
    return None


def fold_transnet_head(params, hyper_params, side, z, emb=None, dtype=torch.float32, head=True):
    """One side of a TransNet's test-time score, source_fm([ue | ie |] project(cat(zu, zi)))[:, 0] (TransNet.py:105-119,
    common_pytorch_models.py:41-57), as the rows of the ReLU-FM form (include/r4r.h):

        score(u, i) = sum_{j<M} y_j (s_j y_j + l_j) + q_bias[u] + c_bias[i]
        y = W x + b,   x_m = relu(qa[u][m] + ca[i][m])  m < H = L,   x_{H+f} = qp[u][f] + cp[i][f]  f < P

    With W0, b0 = source.project.0, W2, b2 = source.project.2, V, lw, lb = source_fm.V, lin.weight[0], lin.bias, R = 8,
    o = 10 (transnet++: the leading rows of V / lw that belong to [user_embedding | item_embedding]) or 0, Vr = V[o:],
    lr = lw[o:], sig_k = sum_f Vr[k][f]^2 and M = R + L + 1:

        qa = W0[:, :L] zu + b0      ca = W0[:, L:] zi
        rows       W over the H ReLU'd inputs    b            s     l
        f < R      (W2^T Vr)^T                   b2^T Vr     +1/2   0       the FM's (x V)_f, squared
        R + k      diag(sqrt(sig)) W2            sqrt(sig) b2 -1/2  0       the FM's x_k^2 (V^2)_k, k < L
        R + L      lr^T W2                       lr . b2      0     1       the FM's linear term
        q_bias = lb                 c_bias = 0

    transnet++ (P = 8): qp = V[0:5]^T ue, cp = V[5:10]^T ie enter row f through W[f][H + f] = 1, and the scalars
    lw[0:5] . ue - 1/2 sum_k ue_k^2 sum_f V[k][f]^2 (the same over ie, V[5:10], lw[5:10]) go to q_bias / c_bias.
    Dropout is the identity in eval mode.  ``params``: the model's parameters by state_dict key; ``z`` [n, L]: the side's
    eval-mode source tower latents; ``emb`` [n, 5]: its id embedding rows (transnet++ only).
    -> side 'user': (rows [n, H + P], q_bias [n], (W [M, H + P], b [M], s [M], l [M])), the last None with ``head=False``
    (the head does not depend on the rows: a caller that holds it need not have it built again);
    side 'item': (rows, c_bias [n]).
    Plain torch on whatever device the inputs live on, computed in float64 and rounded once to ``dtype``."""
    if side not in ('user', 'item'):
        raise ValueError("fold_transnet_head: side must be 'user' or 'item', got %r" % (side,))
    mt = hyper_params['model_type']
    if mt not in ('transnet', 'transnet++'):
        raise ValueError('fold_transnet_head: no ReLU-FM form for %r' % (mt,))
    pp = mt == 'transnet++'
    if (emb is None) == pp:
        raise ValueError('fold_transnet_head: %s takes %s' % (mt, 'z and emb' if pp else 'z alone'))
    f64 = lambda t: t.detach().to(torch.float64)
    W0, b0, W2, b2, V, lw, lb = (f64(params[k]) for k in (
        'source.project.0.weight', 'source.project.0.bias', 'source.project.2.weight', 'source.project.2.bias',
        'source_fm.V', 'source_fm.lin.weight', 'source_fm.lin.bias'))
    if z.dim() != 2 or (pp and (emb.dim() != 2 or emb.shape[0] != z.shape[0] or emb.shape[1] != _TRANSNET_EMB)):
        raise ValueError('fold_transnet_head: z [n, L] and emb [n, %d] do not match' % _TRANSNET_EMB)
    n, L = z.shape
    o = 2 * _TRANSNET_EMB if pp else 0
    R = V.shape[1]
    lw = lw.reshape(-1)
    if tuple(W0.shape) != (L, 2 * L) or tuple(W2.shape) != (L, L) or V.shape[0] != o + L or lw.numel() != o + L:
        raise ValueError('fold_transnet_head: project %s %s / source_fm.V %s do not match latent width %d'
                         % (tuple(W0.shape), tuple(W2.shape), tuple(V.shape), L))
    user = side == 'user'
    x = f64(z)
    rows = x @ (W0[:, :L] if user else W0[:, L:]).T
    bias = torch.zeros(n, dtype=torch.float64, device=z.device)
    if user:
        rows, bias = rows + b0, bias + lb.reshape(())
    if pp:
        e = f64(emb)
        sl = slice(0, _TRANSNET_EMB) if user else slice(_TRANSNET_EMB, o)
        rows = torch.cat([rows, e @ V[sl]], 1)
        bias = bias + e @ lw[sl] - 0.5 * ((e * e) @ (V[sl] * V[sl]).sum(1))
    if not user:
        return rows.to(dtype), bias.to(dtype)
    if not head:
        return rows.to(dtype), bias.to(dtype), None
    Vr, lr = V[o:], lw[o:]
    root = (Vr * Vr).sum(1).sqrt()
    P, M = (R if pp else 0), R + L + 1
    W = torch.zeros((M, L + P), dtype=torch.float64, device=z.device)
    W[:R, :L], W[R:R + L, :L], W[R + L, :L] = (W2.T @ Vr).T, root[:, None] * W2, lr @ W2
    if pp:
        W[torch.arange(R), L + torch.arange(R)] = 1.0
    b = torch.cat([b2 @ Vr, root * b2, (lr @ b2).reshape(1)])
    s = torch.cat([torch.full((R,), 0.5), torch.full((L,), -0.5), torch.zeros(1)]).to(torch.float64).to(z.device)
    l = torch.cat([torch.zeros(R + L), torch.ones(1)]).to(torch.float64).to(z.device)
    return rows.to(dtype), bias.to(dtype), tuple(t.to(dtype).contiguous() for t in (W, b, s, l))


class TransNetCatalogue(Catalogue):
    """``Catalogue``'s surface (``refresh``, ``recommend``, ``score_pairs``, ``rank``; the same return types, devices,
    (-1, -inf) fill and argument checks: the three calls are ``Catalogue``'s own, over this class's ``_head``) for
    transnet and transnet++, ranked by r4r_topk_rfm / r4r_pair_rfm / r4r_rank_rfm.

    At test time a TransNet predicts without the pair's review: source_fm over the source network (TransNet.py:105-119),
    whose towers read the user's and the item's document -- every review of the owner; a rating outside the training
    split removes nothing (data.py:240-246).  ``fold_transnet_head`` has the table.

    ``refresh()`` flushes the engine's pending row updates and caches the item side (``c``, ``c_bias`` with -inf in
    ineligible rows, the head ``W``, ``b``, ``s``, ``l``): the item documents through source.item_conv over
    target.word2vec.weight, ``tower_batch`` at a time.  The query side is computed per call from the current weights.
    A pass leaves the training state untouched.  No CPU and no torch fallback.  ``main``'s hooks do not reach this
    class; the TransNets are served here and through ``eval_catalogue(catalogue=TransNetCatalogue(...))``."""

    _form = 'rfm'
    _limits = staticmethod(transnet_catalogue_limits)

    def _shape(self):
        self.pp = self.mt == 'transnet++'
        L = _latent_size(self.hp)
        self.H, self.P, self.M = L, (FM_RANK if self.pp else 0), FM_RANK + L + 1
        self.D = self.H + self.P
        self.n_c = self.n_items                                # one row per item id

    def _words(self):
        """The source towers read the target network's frozen word table."""
        return self.model.target.word2vec.weight

    def _source(self, side):
        """(pool, source tower, name of the id embedding table) of 'user' / 'item'."""
        src = self.model.source
        return ((self.reader.store.users, src.user_conv, 'user_embedding') if side == 'user' else
                (self.reader.store.items, src.item_conv, 'item_embedding'))

    def _phrase_side(self, side):
        """``explain_words`` reads the SOURCE towers: they are what scores a pair at test time."""
        pool, tower, _ = self._source(side)
        return pool, tower, None

    def _side(self, P, side, ids, sel, z=None):
        """``fold_transnet_head`` of the owners ``ids`` (a host int64 array; ``sel``: the same ids on the device;
        ``z``: their tower latents where the caller holds them)."""
        pool, tower, table = self._source(side)
        if z is None:
            z = self._tower(tower, self._documents(pool, ids))
        emb = getattr(self.model, table).weight.detach()[sel] if self.pp else None
        return fold_transnet_head(P, self.hp, side, z, emb=emb, head=False)      # (the head is refresh()'s)

    def refresh(self):
        self._flush()
        P = self._params()
        elig, _, cb = self._eligible_rows()
        c = torch.zeros((self.n_c, self.D), dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            pool, tower, _ = self._source('item')
            for sl, ids, z in self._latents(tower, pool, self.eligible):
                sel = elig[sl]
                c[sel], cb[sel] = self._side(P, 'item', ids, sel, z=z)
            self.c, self.c_bias = c, cb
            # the head is the user side's; the fold of zero user rows yields it without a tower forward
            none = torch.zeros((0, self.H), dtype=torch.float32, device=self.dev)
            no_emb = torch.zeros((0, _TRANSNET_EMB), dtype=torch.float32, device=self.dev) if self.pp else None
            self.W, self.b, self.s, self.l = fold_transnet_head(P, self.hp, 'user', none, emb=no_emb)[2]

    def _queries(self, u_host):
        """(q [n, H + P], q_bias [n]) of the requested users from the current weights."""
        P = self._params()
        u = u_host.to(self.dev)
        q = torch.empty((u.numel(), self.D), dtype=torch.float32, device=self.dev)
        qb = torch.empty((u.numel(),), dtype=torch.float32, device=self.dev)
        with torch.no_grad():
            pool, tower, _ = self._source('user')
            for sl, ids, z in self._latents(tower, pool, u_host.numpy()):
                q[sl], qb[sl], _ = self._side(P, 'user', ids, u[sl], z=z)
        return q, qb

    def _head(self, q, n, qb):
        return (ptr(q), n, ptr(qb), ptr(self.c), self.n_c, self.D, ptr(self.c_bias), ptr(self.W), ptr(self.b), ptr(self.s),
                ptr(self.l), self.H, self.P, self.M)

    _pair_kind = 'pfm'

    def _pair_head(self, u, i):
        """The TransNets at test time (TransNet.py:25-35, 105-114): source.project and source_fm as they are, and for
        transnet++ the id-embedding rows of the owners; source_fm.lin.bias is the only scalar."""
        m, P = self.model, self._params()
        qb = P['source_fm.lin.bias'].to(torch.float32).reshape(1).expand(u.numel()).contiguous()
        head = dict(W0=P['source.project.0.weight'], b0=P['source.project.0.bias'], W2=P['source.project.2.weight'],
                    b2=P['source.project.2.bias'], V=P['source_fm.V'], lw=P['source_fm.lin.weight'].reshape(-1), q_bias=qb)
        if self.pp:
            head.update(xu=getattr(m, self._source('user')[2]).weight.detach()[u].contiguous(),
                        xi=getattr(m, self._source('item')[2]).weight.detach()[i].contiguous())
        return head


PFM_MAX_L = 64                      # r4r_topk_pfm: H <= 64, G <= 64, M <= 128


def mf_catalogue_limits(hyper_params):
    """None when ``MFCatalogue`` can rank this configuration, else the reason it cannot.  (The sibling functions'
    texts for MF -- ``transnet_catalogue_limits``' "no class serves it" among them -- predate this class and are kept as
    they are.)"""
    mt = hyper_params['model_type']
    served = _served_before(mt, 4)
    if served:
        return served
    if mt != 'MF':
        return 'model_type %r has no product-FM form' % (mt,)
    if _latent_size(hyper_params) > PFM_MAX_L:
        return 'latent_size %d > %d' % (_latent_size(hyper_params), PFM_MAX_L)
    return None


def fold_mf_head(params, hyper_params, side, emb, bias=None, dtype=torch.float32, head=True):
    """One side of MF's eval-mode score, final([projection(cat(ue, ie)) | ue * ie]) + the three biases (MF.py:45-50,
    common_pytorch_models.py:41-57), as the rows of the product-FM form (include/r4r.h):

        score(u, i) = sum_{j<M} s_j y_j^2 + sum_{m<D} x_m (g_m x_m + e_m) + q_bias[u] + c_bias[i]
        y = W x + b,   x_m = relu(qa[u][m] + ca[i][m])  m < H = L,   x_{H+f} = ue[u][f] ie[i][f]  f < G = L

    With W1, b1 = projection.1, W3, b3 = projection.3, V, lw, lb = final.V [2 L, L], final.lin.weight[0], final.lin.bias,
    Va = V[:L], Vb = V[L:], la = lw[:L], lm = lw[L:], sig_a = sum_f Va[.][f]^2, sig_b likewise over Vb, D = M = 2 L:

        qa = W1[:, :L] ue + b1      ca = W1[:, L:] ie
        rows       W over h              W over m    b              s
        f < L      (W3^T Va)^T           Vb^T        b3^T Va       +1/2      the FM's (x V)_f, squared
        L + k      diag(sqrt(sig_a)) W3  0           sqrt(sig_a) b3 -1/2     the FM's ir_k^2 (V^2)_k, ir = W3 h + b3
        columns    e = [la^T W3 | lm]    g = [0 | -1/2 sig_b]                the linear term, and m_k^2 (V^2)_{L+k}
        q_bias = user_bias + global_bias + lb + la . b3        c_bias = item_bias

    Dropout is the identity in eval mode.  ``params``: the model's parameters by state_dict key; ``emb`` [n, L]: the
    side's embedding rows; ``bias`` [n]: its rows of user_bias / item_bias (None: zeros).
    -> side 'user': (rows [n, 2 L] = [qa | ue], q_bias [n], (W [2 L, 2 L], b [2 L], s [2 L], g [2 L], e [2 L])), the last
    None with ``head=False`` (the head does not depend on the rows);  side 'item': (rows [n, 2 L] = [ca | ie], c_bias [n]).
    Plain torch on whatever device the inputs live on, computed in float64 and rounded once to ``dtype``."""
    if side not in ('user', 'item'):
        raise ValueError("fold_mf_head: side must be 'user' or 'item', got %r" % (side,))
    if hyper_params['model_type'] != 'MF':
        raise ValueError('fold_mf_head: no product-FM form for %r' % (hyper_params['model_type'],))
    f64 = lambda t: t.detach().to(torch.float64)
    W1, b1, W3, b3, V, lw, lb, gb = (f64(params[k]) for k in (
        'projection.1.weight', 'projection.1.bias', 'projection.3.weight', 'projection.3.bias', 'final.V',
        'final.lin.weight', 'final.lin.bias', 'global_bias'))
    if emb.dim() != 2 or (bias is not None and (bias.dim() != 1 or bias.shape[0] != emb.shape[0])):
        raise ValueError('fold_mf_head: emb [n, L] and bias [n] do not match')
    n, L = emb.shape
    lw = lw.reshape(-1)
    if tuple(W1.shape) != (L, 2 * L) or tuple(W3.shape) != (L, L) or tuple(V.shape) != (2 * L, L) or lw.numel() != 2 * L:
        raise ValueError('fold_mf_head: projection %s %s / final.V %s do not match latent width %d'
                         % (tuple(W1.shape), tuple(W3.shape), tuple(V.shape), L))
    user = side == 'user'
    x = f64(emb)
    sc = torch.zeros(n, dtype=torch.float64, device=emb.device) if bias is None else f64(bias)
    la, lm = lw[:L], lw[L:]
    if not user:
        return torch.cat([x @ W1[:, L:].T, x], 1).to(dtype), sc.to(dtype)
    rows = torch.cat([x @ W1[:, :L].T + b1, x], 1)
    sc = sc + gb.reshape(()) + lb.reshape(()) + la @ b3
    if not head:
        return rows.to(dtype), sc.to(dtype), None
    Va, Vb = V[:L], V[L:]
    root = (Va * Va).sum(1).sqrt()
    zero = torch.zeros((L, L), dtype=torch.float64, device=emb.device)
    W = torch.cat([torch.cat([(W3.T @ Va).T, Vb.T], 1), torch.cat([root[:, None] * W3, zero], 1)], 0)
    b = torch.cat([b3 @ Va, root * b3])
    s = torch.cat([torch.full((L,), 0.5), torch.full((L,), -0.5)]).to(torch.float64).to(emb.device)
    g = torch.cat([zero[0], -0.5 * (Vb * Vb).sum(1)])
    e = torch.cat([la @ W3, lm])
    return rows.to(dtype), sc.to(dtype), tuple(t.to(dtype).contiguous() for t in (W, b, s, g, e))


class MFCatalogue(Catalogue):
    """``Catalogue``'s surface (``refresh``, ``recommend``, ``score_pairs``, ``rank``; the same return types, devices,
    (-1, -inf) fill and argument checks: the three calls are ``Catalogue``'s own, over this class's ``_head``) for MF,
    ranked by r4r_topk_pfm / r4r_pair_pfm / r4r_rank_pfm.  ``fold_mf_head`` has the table.

    ``refresh()`` flushes the engine's pending row updates (the blocked sweeps of the native step leave table rows
    behind the schedule until ``flush()``) and caches the item side (``c`` = [ca | ie], ``c_bias`` = item_bias with -inf
    in ineligible rows, the head ``W``, ``b``, ``s``, ``g``, ``e``): the item table through one small matmul, no tower
    and no document.  The query side is computed per call from the current weights, after the same flush.  A pass leaves
    the training state untouched.  No CPU and no torch fallback.  ``main``'s hooks do not reach this class (they still
    refuse MF, and ``transnet_catalogue_limits`` still says that no class serves it: both texts are older than this
    class); MF is served here and through ``eval_catalogue(catalogue=MFCatalogue(...))``."""

    _form = 'pfm'
    _limits = staticmethod(mf_catalogue_limits)

    def __init__(self, model, hyper_params, train_reader, engine=None, candidates=None):
        super().__init__(model, hyper_params, train_reader, engine=engine, candidates=candidates)
        del self.tower_batch                                   # no tower, nothing to batch

    def _shape(self):
        L = _latent_size(self.hp)
        self.H, self.G, self.M = L, L, 2 * L
        self.D = self.H + self.G
        self.n_c = int(self.model.item_bias.numel())           # the item table as it is

    def refresh(self):
        self._flush()
        m, P = self.model, self._params()
        _, mask, ninf = self._eligible_rows()
        with torch.no_grad():
            c, cb = fold_mf_head(P, self.hp, 'item', m.item_embedding.weight.detach(), bias=m.item_bias.detach())
            self.c, self.c_bias = c.contiguous(), torch.where(mask, cb, ninf)
            # the head is the user side's; the fold of zero user rows yields it
            none = torch.zeros((0, self.H), dtype=torch.float32, device=self.dev)
            self.W, self.b, self.s, self.g, self.e = fold_mf_head(P, self.hp, 'user', none)[2]

    def _queries(self, u_host):
        """(q [n, 2 L], q_bias [n]) of the requested users from the current weights."""
        self._flush()
        m = self.model
        u = u_host.to(self.dev)
        with torch.no_grad():
            q, qb, _ = fold_mf_head(self._params(), self.hp, 'user', m.user_embedding.weight.detach()[u],
                                    bias=m.user_bias.detach()[u], head=False)
        return q.contiguous(), qb.contiguous()

    def _head(self, q, n, qb):
        return (ptr(q), n, ptr(qb), ptr(self.c), self.n_c, self.D, ptr(self.c_bias), ptr(self.W), ptr(self.b), ptr(self.s),
                ptr(self.g), ptr(self.e), self.H, self.G, self.M)


def hook_limits(hyper_params):
    """None when ``make_catalogue`` can serve main's hooks for this configuration, else the reason: ``catalogue_limits``'
    for every type but deepconn++, which ``ReluCatalogue`` serves (NeuMF goes through the class, not through main)."""
    why = catalogue_limits(hyper_params)
    if why is None or hyper_params['model_type'] != 'deepconn++':
        return why
    return relu_catalogue_limits(hyper_params)


def make_catalogue(model, hyper_params, train_reader, engine=None):
    """The class that serves main's hooks: ``Catalogue`` where ``catalogue_limits`` accepts, else ``ReluCatalogue``."""
    cls = Catalogue if catalogue_limits(hyper_params) is None else ReluCatalogue
    return cls(model, hyper_params, train_reader, engine=engine, towers=hyper_params.get('catalogue_towers', 'host'))


def ranking_metrics(ranks, ks):
    """Full-catalogue metrics of 0-based ``ranks`` (``Catalogue.rank``; -1 = the item cannot be ranked: no training
    rating, so the catalogue does not hold it), on the host in float64, nothing rounded:

        HR@k = mean(rank < k)    NDCG@k = mean(1 / log2(rank + 2) where rank < k, else 0)    MRR = mean(1 / (rank + 1))

    over the ranked pairs only; ``ranked`` / ``unranked`` report both counts.  No ranked pair: ZeroDivisionError."""
    r = ranks.detach().cpu().numpy() if isinstance(ranks, torch.Tensor) else np.asarray(ranks)
    r = r.reshape(-1).astype(np.int64)
    ks = [int(k) for k in ks]
    if any(k < 1 for k in ks):
        raise ValueError('ranking_metrics: every k must be positive, got %r' % (ks,))
    ok = r[r >= 0].astype(np.float64)
    n = int(len(ok))
    out = {'ranked': n, 'unranked': int(len(r)) - n}
    gain = 1.0 / np.log2(ok + 2.0)
    for k in ks:
        hit = ok < k
        out['HR@%d' % k] = float(hit.sum()) / n                # (n == 0: ZeroDivisionError, like eval.py:90)
        out['NDCG@%d' % k] = float(gain[hit].sum()) / n
    out['MRR'] = float((1.0 / (ok + 1.0)).sum()) / n
    return out


def _check_towers_request(hyper_params):
    """hyper_params['catalogue_towers'] (``Catalogue``'s ``towers``; absent: 'host') of a request main's hooks will serve."""
    towers = hyper_params.get('catalogue_towers', 'host')
    if towers not in TOWERS:
        raise RuntimeError("hyper_params['catalogue_towers'] must be one of %r, got %r" % (TOWERS, towers))


def check_catalogue_metrics_request(hyper_params):
    """main's hook asked for (hyper_params['catalogue_metrics_k'])?  Then refuse, BEFORE anything is loaded, a list that
    is not a non-empty list of positive ints and a model type without a catalogue form (``catalogue_limits``' reason)."""
    if hyper_params.get('catalogue_metrics_k') is None:
        return
    ks = hyper_params['catalogue_metrics_k']
    if (not isinstance(ks, (list, tuple)) or len(ks) == 0 or
            any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 for k in ks)):
        raise RuntimeError("hyper_params['catalogue_metrics_k'] must be a non-empty list of positive ints, got %r" % (ks,))
    why_not = hook_limits(hyper_params)
    if why_not is not None:
        raise RuntimeError("hyper_params['catalogue_metrics_k']: " + why_not)
    _check_towers_request(hyper_params)


def check_recommend_request(hyper_params):
    """main's hook asked for (hyper_params['recommend_k'])?  Then refuse, BEFORE any training, a model type without a
    catalogue form and a request without a file to write."""
    if not hyper_params.get('recommend_k'):
        return
    why_not = hook_limits(hyper_params)
    if why_not is not None:
        raise RuntimeError("hyper_params['recommend_k']: " + why_not)
    if not hyper_params.get('recommend_path'):
        raise RuntimeError("hyper_params['recommend_k'] needs hyper_params['recommend_path'] (the .npz to write)")
    _check_towers_request(hyper_params)


def write_recommendations(path, model, hyper_params, train_reader, k, engine=None):
    """main.main's hook: the top-k list of every user with a training rating -> an .npz of users / items / scores."""
    cat = make_catalogue(model, hyper_params, train_reader, engine=engine)
    users = np.array(sorted(int(u) for u in train_reader.user_count), dtype=np.int64)
    items, scores = cat.recommend(users, k=int(k))
    with open(path, 'wb') as f:                              # (a file object: numpy appends no suffix to the name)
        np.savez(f, users=users, items=items.cpu().numpy(), scores=scores.cpu().numpy())
    return path


def check_explain_request(hyper_params):
    """main's hook asked for (hyper_params['explain_k'])?  Then refuse, BEFORE any training, a configuration
    ``NarreCatalogue`` cannot serve (``narre_catalogue_limits``' reason: only NARRE has review-level attention), a k
    that is no int in 1 .. narre_num_reviews and a request without a file to write."""
    if not hyper_params.get('explain_k'):
        return
    why_not = narre_catalogue_limits(hyper_params)
    if why_not is not None:
        raise RuntimeError("hyper_params['explain_k']: " + why_not)
    k, R = hyper_params['explain_k'], int(hyper_params.get('narre_num_reviews', NEIGHBOURS))
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= R:
        raise RuntimeError("hyper_params['explain_k'] must be an int in 1 .. narre_num_reviews = %d, got %r" % (R, k))
    if not hyper_params.get('explain_path'):
        raise RuntimeError("hyper_params['explain_k'] needs hyper_params['explain_path'] (the .npz to write)")
    _check_towers_request(hyper_params)


def write_explanations(path, model, hyper_params, train_reader, k, engine=None):
    """main.main's hook: the k most useful reviews of every eligible item (``NarreCatalogue.explain``) -> an .npz of
    items / slots / reviews / reviewers / weights."""
    cat = NarreCatalogue(model, hyper_params, train_reader, engine=engine,
                         towers=hyper_params.get('catalogue_towers', 'host'))
    e = cat.explain(cat.eligible, k=int(k), side='item')
    with open(path, 'wb') as f:                              # (a file object: numpy appends no suffix to the name)
        np.savez(f, items=cat.eligible, slots=e.slots.cpu().numpy(), reviews=e.reviews.cpu().numpy(),
                 reviewers=e.reviewers.cpu().numpy(), weights=e.weights.cpu().numpy())
    return path


def _phrase_class(hyper_params):
    """The class whose ``explain_words`` serves this model type (``phrase_limits`` accepted it)."""
    mt = hyper_params['model_type']
    return {'deepconn': Catalogue, 'deepconn++': ReluCatalogue, 'NARRE': NarreCatalogue}.get(mt, TransNetCatalogue)


def check_explain_words_request(hyper_params):
    """main's hook asked for (hyper_params['explain_words_k'])?  Then refuse, BEFORE any training, a model type without
    a TextCNN tower (``phrase_limits``' reason) or that its class cannot serve, a k that is no int in 1 .. 100 (the
    towers' filter count), a request without a file to write and an unknown ``catalogue_towers``."""
    if not hyper_params.get('explain_words_k'):
        return
    why_not = phrase_limits(hyper_params) or _phrase_class(hyper_params)._limits(hyper_params)
    if why_not is not None:
        raise RuntimeError("hyper_params['explain_words_k']: " + why_not)
    k = hyper_params['explain_words_k']
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= PHRASE_FILTERS:
        raise RuntimeError("hyper_params['explain_words_k'] must be an int in 1 .. %d, got %r" % (PHRASE_FILTERS, k))
    if not hyper_params.get('explain_words_path'):
        raise RuntimeError("hyper_params['explain_words_k'] needs hyper_params['explain_words_path'] (the .npz to write)")
    _check_towers_request(hyper_params)


def write_phrases(path, model, hyper_params, train_reader, k, engine=None):
    """main.main's hook: the k heaviest word windows of every eligible item (``explain_words``; NARRE: of each of its R
    reviews) -> an .npz of items / positions / scores / filters / tokens / reviews / offsets."""
    cat = _phrase_class(hyper_params)(model, hyper_params, train_reader, engine=engine,
                                      towers=hyper_params.get('catalogue_towers', 'host'))
    p = cat.explain_words(cat.eligible, k=int(k), side='item')
    with open(path, 'wb') as f:                              # (a file object: numpy appends no suffix to the name)
        np.savez(f, items=cat.eligible, positions=p.positions.cpu().numpy(), scores=p.scores.cpu().numpy(),
                 filters=p.filters.cpu().numpy(), tokens=p.tokens.cpu().numpy(), reviews=p.reviews.cpu().numpy(),
                 offsets=p.offsets.cpu().numpy())
    return path


def check_explain_pairs_request(hyper_params):
    """main's hook asked for (hyper_params['explain_pairs_k'])?  Then refuse, BEFORE any training, a model type the
    hooks' classes cannot explain (``phrase_limits``' reason, else ``hook_limits``': deepconn and deepconn++ are the types
    ``make_catalogue`` serves), a k that is no int in 1 .. 100 (the towers' filter count), a request without a file to
    write, one without ``recommend_k`` (the pairs explained are the recommended ones) and an unknown ``catalogue_towers``."""
    if not hyper_params.get('explain_pairs_k'):
        return
    why_not = phrase_limits(hyper_params) or hook_limits(hyper_params)
    if why_not is not None:
        raise RuntimeError("hyper_params['explain_pairs_k']: " + why_not)
    k = hyper_params['explain_pairs_k']
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= PHRASE_FILTERS:
        raise RuntimeError("hyper_params['explain_pairs_k'] must be an int in 1 .. %d, got %r" % (PHRASE_FILTERS, k))
    if not hyper_params.get('explain_pairs_path'):
        raise RuntimeError("hyper_params['explain_pairs_k'] needs hyper_params['explain_pairs_path'] (the .npz to write)")
    if not hyper_params.get('recommend_k'):
        raise RuntimeError("hyper_params['explain_pairs_k'] needs hyper_params['recommend_k']: the pairs it explains are "
                           "every user's recommended items")
    _check_towers_request(hyper_params)


def recommended_pairs(cat, k):
    """(users, items) int64 host arrays: every training user's ``recommend(k)`` list, row-major, unused slots dropped."""
    users = np.array(sorted(int(u) for u in cat.reader.user_count), dtype=np.int64)
    items = cat.recommend(users, k=int(k))[0].cpu().numpy()
    keep = items >= 0
    return np.repeat(users, items.shape[1]).reshape(items.shape)[keep], items[keep]


def write_pair_phrases(path, model, hyper_params, train_reader, k, engine=None):
    """main.main's hook: ``explain_pair`` ('up') of every training user's ``recommend_k`` list -> an .npz whose rows are
    the n pairs' user sides followed by the n pairs' item sides: users / items (the row's pair), side (0: the windows of
    the user's reviews, 1: of the item's), pair_scores (the pair's prediction), and ``write_phrases``' positions / scores
    / filters / tokens / reviews / offsets of that side."""
    cat = make_catalogue(model, hyper_params, train_reader, engine=engine)
    users, items = recommended_pairs(cat, hyper_params['recommend_k'])
    e = cat.explain_pair(users, items, k=int(k))
    both = lambda name: np.concatenate([getattr(e.user, name).cpu().numpy(), getattr(e.item, name).cpu().numpy()])
    n = len(users)
    with open(path, 'wb') as f:                              # (a file object: numpy appends no suffix to the name)
        np.savez(f, users=np.tile(users, 2), items=np.tile(items, 2), side=np.repeat(np.array([0, 1], np.int8), n),
                 pair_scores=np.tile(e.scores.cpu().numpy(), 2), positions=both('positions'), scores=both('scores'),
                 filters=both('filters'), tokens=both('tokens'), reviews=both('reviews'), offsets=both('offsets'))
    return path


def check_explain_reviews_request(hyper_params):
    """main's hook asked for (hyper_params['explain_reviews_k'])?  Then refuse, BEFORE any training, a model type the
    hooks' classes cannot explain (``phrase_limits``' reason, else ``hook_limits``': deepconn and deepconn++), a k that
    is no int in 1 .. 64 (the reviews of an owner that can be removed), a request without a file to write, one without
    ``recommend_k`` (the pairs explained are the recommended ones) and an unknown ``catalogue_towers``."""
    if not hyper_params.get('explain_reviews_k'):
        return
    why_not = phrase_limits(hyper_params) or hook_limits(hyper_params)
    if why_not is None and hyper_params['model_type'] not in ('deepconn', 'deepconn++'):
        why_not = ('model_type %r: the hook removes reviews from the single-document families deepconn and deepconn++ '
                   '(NARRE: NarreCatalogue.leave_one_out)' % (hyper_params['model_type'],))
    if why_not is not None:
        raise RuntimeError("hyper_params['explain_reviews_k']: " + why_not)
    k = hyper_params['explain_reviews_k']
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 1 <= k <= WHATIF_MAX_SLOTS:
        raise RuntimeError("hyper_params['explain_reviews_k'] must be an int in 1 .. %d, got %r" % (WHATIF_MAX_SLOTS, k))
    if not hyper_params.get('explain_reviews_path'):
        raise RuntimeError("hyper_params['explain_reviews_k'] needs hyper_params['explain_reviews_path'] (the .npz to "
                           "write)")
    if not hyper_params.get('recommend_k'):
        raise RuntimeError("hyper_params['explain_reviews_k'] needs hyper_params['recommend_k']: the pairs it explains "
                           "are every user's recommended items")
    _check_towers_request(hyper_params)


def top_removed_reviews(loo, k):
    """Per pair and side of a ``DocLeaveOneOut`` the ``k`` reviews whose removal LOWERS the prediction most (the largest
    delta first, ties to the earlier review; only slots that hold a review) -> (reviews int64 [2, n, k] with -1 unused,
    deltas float32 [2, n, k] with 0 there) as host arrays, side 0 the user's."""
    out_r, out_d = [], []
    for delta, live in ((loo.delta_user, loo.live_user), (loo.delta_item, loo.live_item)):
        n, S = delta.shape
        pad = max(0, k - S)
        d = torch.cat([delta, delta.new_zeros((n, pad))], 1)
        valid = torch.arange(S + pad, device=delta.device)[None, :] < live[:, None]
        order = torch.sort(torch.where(valid, d, torch.full_like(d, float('-inf'))), dim=1, descending=True,
                           stable=True).indices[:, :k]
        ok = valid.gather(1, order)
        out_r.append(torch.where(ok, order, torch.full_like(order, -1)).cpu().numpy())
        out_d.append(torch.where(ok, d.gather(1, order), torch.zeros_like(d[:, :k])).cpu().numpy())
    return np.stack(out_r), np.stack(out_d)


def write_pair_reviews(path, model, hyper_params, train_reader, k, engine=None):
    """main.main's hook: ``leave_one_out`` of every training user's ``recommend_k`` list -> an .npz whose rows are the n
    pairs' user sides followed by the n pairs' item sides: users / items (the row's pair), side (0: the user's reviews,
    1: the item's), pair_scores (the pair's prediction), reviews (the k reviews whose removal lowers the prediction
    most, as indices into the side's pool order of the owner; -1 unused) and deltas (base - without of each)."""
    cat = make_catalogue(model, hyper_params, train_reader, engine=engine)
    users, items = recommended_pairs(cat, hyper_params['recommend_k'])
    loo = cat.leave_one_out(users, items)
    reviews, deltas = top_removed_reviews(loo, int(k))
    n = len(users)
    with open(path, 'wb') as f:                              # (a file object: numpy appends no suffix to the name)
        np.savez(f, users=np.tile(users, 2), items=np.tile(items, 2), side=np.repeat(np.array([0, 1], np.int8), n),
                 pair_scores=np.tile(loo.base.cpu().numpy(), 2), reviews=reviews.reshape(2 * n, -1),
                 deltas=deltas.reshape(2 * n, -1))
    return path
