"""Catalogue recommendation on the device: r4r_topk_dot (csrc/topk.hip, include/r4r.h "Catalogue recommendation") and
recommend.Catalogue on top of it.

The reference ordering lives here: float64 scores, np.lexsort on (id, -score), the exclusions applied, the -1 / -inf
fill.  With inputs that are multiples of 1/8 (biases: of 1/64) every partial sum is exact in fp32 for D <= 256, so the
kernel must return EXACTLY that list, ids and score bits; with real-valued inputs the a-priori bound of the fixed
expression, (D + 3) 2^-24 (sum_j |q_j c_j| + |c_bias| + |q_bias|), decides what is demanded (equal ids where the float64
gaps exceed twice the bound, a valid list elsewhere)."""
import os

import numpy as np
import pytest
import torch

from helpers import materialise_tiny, tiny_hp

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EPS = 2.0 ** -24


# ---------------------------------------------------------------- the reference ordering
def ref_scores(q, qb, c, cb):
    s = q.astype(np.float64) @ c.astype(np.float64).T
    with np.errstate(invalid='ignore'):
        if cb is not None:
            s = s + cb.astype(np.float64)[None, :]
        if qb is not None:
            s = s + qb.astype(np.float64)[:, None]
    return s


def mask_excluded(s, excl):
    s = s.copy()
    if excl is not None:
        off, ids = excl
        for u in range(s.shape[0]):
            s[u, ids[off[u]:off[u + 1]]] = -np.inf
    return s


def ref_lists(s, K):
    """s: float64 [n_q, n_c], -inf / NaN = never returned -> (ids int64 [n_q, K], scores float64 [n_q, K])."""
    n_q = s.shape[0]
    ids = np.full((n_q, K), -1, np.int64)
    sc = np.full((n_q, K), -np.inf, np.float64)
    for u in range(n_q):
        with np.errstate(invalid='ignore'):
            idx = np.nonzero(s[u] > -np.inf)[0]
        top = idx[np.lexsort((idx, -s[u, idx]))][:K]
        ids[u, :len(top)] = top
        sc[u, :len(top)] = s[u, top]
    return ids, sc


# ---------------------------------------------------------------- the call
def topk(q, qb, c, cb, K, chunk=0, excl=None, pad=3):
    """r4r_topk_dot over numpy inputs; c goes to the device with a row stride of D + pad (the pad holds NaN)."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    n_q, D = q.shape
    n_c = c.shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    cs = torch.full((max(n_c, 1), D + pad), float('nan'), dtype=torch.float32, device=DEV)
    if n_c and D:
        cs[:n_c, :D] = dev(c)
    qd, qbd, cbd = dev(q.reshape(-1) if D else np.zeros(1, np.float32)), dev(qb), dev(cb)
    eo, ei = (None, None) if excl is None else (dev(excl[0]), dev(np.concatenate([excl[1], np.zeros(1, np.int64)])))
    ids = torch.full((n_q, K), -7, dtype=torch.int64, device=DEV)
    sc = torch.full((n_q, K), 7.0, dtype=torch.float32, device=DEV)
    lib = _lib.lib()
    nb = lib.r4r_topk_dot_ws_bytes(n_q, n_c, K, chunk)
    ws = torch.empty(max(int(nb), 16), dtype=torch.uint8, device=DEV)
    _lib.call('r4r_topk_dot', ptr(qd), n_q, ptr(qbd), ptr(cs), n_c, D + pad, ptr(cbd), D, ptr(eo), ptr(ei), K, chunk,
              ptr(ws), int(nb), ptr(ids), ptr(sc))
    torch.cuda.synchronize()
    return ids.cpu().numpy(), sc.cpu().numpy()


def small_chunk(n_c):
    """A forced chunk with at least three partial lists and a ragged last one (where n_c allows it)."""
    for ch in range(max(1, n_c // 3), 0, -1):
        if n_c % ch and -(-n_c // ch) >= 3:
            return ch
    return 1


def dyadic(rng, shape, step, lim):
    return (rng.integers(-int(lim / step), int(lim / step) + 1, size=shape) * step).astype(np.float32)


# ---------------------------------------------------------------- 1. exact arithmetic
N_Q, N_C = [1, 15, 16, 17, 33], [1, 15, 16, 17, 255, 257, 4099]
DS, KS = [0, 1, 3, 4, 5, 8, 64, 100, 256], [1, 5, 10, 128]
EXACT = sorted({(N_Q[t % 5], N_C[(3 * t) % 7], DS[t % 9], KS[t % 4]) for t in range(36)} |
               {(33, 4099, 256, 128), (33, 4099, 64, 10), (17, 4099, 100, 128), (16, 257, 8, 10), (1, 4099, 0, 5),
                (33, 255, 0, 128), (17, 16, 256, 5), (15, 4099, 5, 1),
                # from 512 queries on a wave holds 64 of them (four accumulator tiles) while D <= 128
                (511, 257, 5, 5), (512, 4099, 64, 10), (577, 1000, 128, 128), (513, 300, 256, 5), (600, 255, 0, 1)})


@pytest.mark.parametrize('n_q, n_c, D, K', EXACT)
def test_exact_inputs_give_the_reference_list_bit_for_bit(n_q, n_c, D, K):
    assert 40 <= len(EXACT) <= 52
    rng = np.random.default_rng(n_q * 1000003 + n_c * 131 + D * 7 + K)
    q, c = dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_c, D), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 0.25)      # (narrow: plenty of exact ties)
    want_ids, want_sc = ref_lists(ref_scores(q, qb, c, cb), K)
    assert np.array_equal(want_sc.astype(np.float32).astype(np.float64), want_sc)     # exact in fp32
    for chunk in (0, small_chunk(n_c)):
        ids, sc = topk(q, qb, c, cb, K, chunk)
        assert np.array_equal(ids, want_ids), (chunk, np.argwhere(ids != want_ids)[:5])
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk
    if K == 5:                                                                        # NULL biases count as 0
        ids, sc = topk(q, None, c, None, K, small_chunk(n_c))
        want_ids, want_sc = ref_lists(ref_scores(q, None, c, None), K)
        assert np.array_equal(ids, want_ids) and np.array_equal(sc, want_sc.astype(np.float32))


# ---------------------------------------------------------------- 2. degenerate rankings
@pytest.mark.parametrize('case', ['all equal', 'K above the eligible count', 'every candidate -inf', 'a NaN row'])
def test_degenerate_rankings(case):
    rng = np.random.default_rng(5)
    n_q, n_c, D, K = 17, 300, 8, 10
    q, c = dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_c, D), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 1.0)
    if case == 'all equal':
        c[:], cb[:] = 0.0, 0.5
    elif case == 'K above the eligible count':
        cb[rng.permutation(n_c)[7:]] = -np.inf                                       # seven eligible rows
    elif case == 'every candidate -inf':
        cb[:] = -np.inf
    else:
        c[41], c[42, 3] = np.nan, np.nan
        q[0] = 0.0                                                                   # 0 * NaN is NaN all the same
        cb[43] = np.nan
    want_ids, want_sc = ref_lists(ref_scores(q, qb, c, cb), K)
    if case == 'all equal':
        assert (want_ids == np.arange(K)[None, :]).all()
    if case == 'K above the eligible count':
        assert (want_ids[:, 7:] == -1).all() and (want_ids[:, :7] >= 0).all()
    if case == 'every candidate -inf':
        assert (want_ids == -1).all()
    if case == 'a NaN row':
        assert not np.isin(want_ids, [41, 42, 43]).any()
    for chunk in (0, 64, 7):
        ids, sc = topk(q, qb, c, cb, K, chunk)
        assert np.array_equal(ids, want_ids), (case, chunk)
        assert np.array_equal(sc, want_sc.astype(np.float32)), (case, chunk)


# ---------------------------------------------------------------- 3. exclusions
def test_exclusions():
    rng = np.random.default_rng(6)
    n_q, n_c, D, K = 5, 1000, 8, 10
    q, c = dyadic(rng, (n_q, D), 0.125, 1.0), dyadic(rng, (n_c, D), 0.125, 1.0)
    qb, cb = dyadic(rng, (n_q,), 1 / 64, 2.0), dyadic(rng, (n_c,), 1 / 64, 1.0)
    s = ref_scores(q, qb, c, cb)
    free_ids, _ = ref_lists(s, K)
    lists = [np.zeros(0, np.int64),                                                  # an empty list
             free_ids[1, :1].copy(),                                                 # the best candidate
             np.arange(n_c, dtype=np.int64),                                         # everything
             np.sort(rng.permutation(n_c)[:300]).astype(np.int64),                   # long, across every chunk boundary
             np.sort(free_ids[4]).astype(np.int64)]                                  # the whole free top-K
    lists[3] = np.union1d(lists[3], free_ids[3, :4]).astype(np.int64)
    off = np.zeros(n_q + 1, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    excl = (off, np.concatenate(lists))
    want_ids, want_sc = ref_lists(mask_excluded(s, excl), K)
    assert np.array_equal(want_ids[0], free_ids[0]) and want_ids[1, 0] == free_ids[1, 1]
    assert (want_ids[2] == -1).all() and not np.isin(want_ids[3], lists[3]).any()
    assert not np.isin(want_ids[4], free_ids[4]).any()
    for chunk in (0, 64, 333):
        ids, sc = topk(q, qb, c, cb, K, chunk, excl=excl)
        assert np.array_equal(ids, want_ids), chunk
        assert np.array_equal(sc, want_sc.astype(np.float32)), chunk


# ---------------------------------------------------------------- 4. real-valued inputs
def check_lists(ids, sc, s64, tol, K, what=''):
    """ids / sc [n_q, K] against float64 scores s64 [n_q, n_c] (-inf / NaN: never returned) and the per-pair bound tol
    [n_q, n_c]: a list is VALID when it has min(K, eligible) distinct eligible ids in the kernel's own order, every score
    within its bound, and no item below the float64 K-th best by more than twice the row's largest bound; where the
    float64 gaps around the list exceed that, the ids must be the reference's.  -> rows whose ids were demanded."""
    want_ids, want_sc = ref_lists(s64, K)
    demanded = 0
    for u in range(ids.shape[0]):
        with np.errstate(invalid='ignore'):
            ok = s64[u] > -np.inf
        n = min(K, int(ok.sum()))
        got = ids[u, :n]
        assert (ids[u, n:] == -1).all() and np.isneginf(sc[u, n:]).all(), (what, u)
        assert (got >= 0).all() and len(set(got.tolist())) == n and ok[got].all(), (what, u, got)
        assert (np.abs(sc[u, :n].astype(np.float64) - s64[u, got]) <= tol[u, got]).all(), (what, u)
        for a in range(n - 1):                                # the returned order is the fp32 order, ties by id
            assert sc[u, a] > sc[u, a + 1] or (sc[u, a] == sc[u, a + 1] and got[a] < got[a + 1]), (what, u, a)
        if n == 0:
            continue
        row_tol = float(tol[u, ok].max())
        assert (s64[u, got] >= want_sc[u, n - 1] - 2 * row_tol).all(), (what, u)
        ranked = np.sort(s64[u, ok])[::-1][:n + 1]
        if len(ranked) < 2 or (ranked[:-1] - ranked[1:]).min() > 2 * row_tol:
            assert np.array_equal(got, want_ids[u, :n]), (what, u)
            demanded += 1
    return demanded


def dot_bound(q, qb_terms, c, cb, D):
    """(D + 3) 2^-24 (sum_j |q_j c_j| + |c_bias| + the |q_bias| terms): D fma roundings, the two additions, and one
    for a q_bias that is itself an fp32 sum (qb_terms: [n_q] = the sum of its terms' magnitudes)."""
    M = np.abs(q.astype(np.float64)) @ np.abs(c.astype(np.float64)).T
    with np.errstate(invalid='ignore'):
        M = M + np.where(np.isfinite(cb), np.abs(cb.astype(np.float64)), 0.0)[None, :] + qb_terms.astype(np.float64)[:, None]
    return (D + 3) * EPS * M


def real_inputs(D, n_q=33, n_c=4099, seed=0):
    rng = np.random.default_rng(100 + D + seed)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)
    return f(n_q, D), f(n_q), f(n_c, D), f(n_c)


@pytest.mark.parametrize('D', [1, 10, 64, 256])
def test_real_valued_inputs_within_the_a_priori_bound(D):
    K = 10
    q, qb, c, cb = real_inputs(D)
    s64 = ref_scores(q, qb, c, cb)
    tol = dot_bound(q, np.abs(qb), c, cb, D)
    for chunk in (0, small_chunk(4099)):
        ids, sc = topk(q, qb, c, cb, K, chunk)
        demanded = check_lists(ids, sc, s64, tol, K, 'D=%d chunk=%d' % (D, chunk))
        assert demanded >= 20, demanded                       # (the emulated fp32 order equalled float64's on every row)


@pytest.mark.parametrize('D', [0, 3, 10, 64, 256])
def test_pair_scores_have_the_bits_of_the_ranking(D):
    """r4r_pair_dot is the scalar fmaf chain; the ranking's MFMA scores must be the same bits (include/r4r.h)."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    K = 10
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    # (against 65 candidates: 256 pairs fill the last 256-thread workgroup of the pair kernel exactly, 257 leave one pair
    # in it)
    for n_c, counts in ((4099, (33 * K,)), (65, (256, 257))):
        q, qb, c, cb = real_inputs(D, n_c=n_c, seed=1)
        ids, sc = topk(q, qb, c, cb, K, 0, pad=0)
        assert (ids >= 0).all()
        qd, cd = dev(q if D else np.zeros((33, 1), np.float32)), dev(c if D else np.zeros((n_c, 1), np.float32))
        qbd, cbd = dev(qb), dev(cb)
        for n in counts:
            qi = dev(np.repeat(np.arange(33, dtype=np.int64), K)[:n])
            ci = dev(ids.reshape(-1)[:n])
            out = torch.full((33 * K,), 7.0, dtype=torch.float32, device=DEV)
            _lib.call('r4r_pair_dot', ptr(qd), 33, ptr(qbd), ptr(cd), n_c, D, ptr(cbd), D, ptr(qi), ptr(ci), n, ptr(out))
            out = out.cpu().numpy()
            assert np.array_equal(out[:n].view(np.uint32), sc.reshape(-1)[:n].view(np.uint32)), (n_c, n)
            assert (out[n:] == 7.0).all(), (n_c, n)                  # nothing is written past the last pair


# ---------------------------------------------------------------- 5. batching invariance
@pytest.mark.parametrize('D', [10, 64, 256])
def test_batching_and_chunking_do_not_change_a_bit(D):
    K = 10
    q, qb, c, cb = real_inputs(D, seed=2)
    rng = np.random.default_rng(D)
    lists = [np.sort(rng.permutation(4099)[:rng.integers(0, 40)]).astype(np.int64) for _ in range(33)]
    off = np.zeros(34, np.int64)
    np.cumsum([len(l) for l in lists], out=off[1:])
    ids_all = np.concatenate(lists)

    def sub(a, b):
        return (off[a:b + 1] - off[a], ids_all[off[a]:off[b]])

    want = topk(q, qb, c, cb, K, 0, excl=sub(0, 33))
    bits = lambda r: (r[0], r[1].view(np.uint32))
    for chunk in (500, 4099):
        got = topk(q, qb, c, cb, K, chunk, excl=sub(0, 33))
        assert all(np.array_equal(x, y) for x, y in zip(bits(got), bits(want))), chunk
        halves = [topk(q[a:b], qb[a:b], c, cb, K, chunk, excl=sub(a, b)) for a, b in ((0, 17), (17, 33))]
        singles = [topk(q[u:u + 1], qb[u:u + 1], c, cb, K, chunk, excl=sub(u, u + 1)) for u in range(33)]
        for parts in (halves, singles):
            got = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]))
            assert all(np.array_equal(x, y) for x, y in zip(bits(got), bits(want))), chunk
    # ... and inside a call of 545 queries, which runs the 64-query tiles where D <= 128
    more = np.random.default_rng(D + 1).standard_normal((512, D)).astype(np.float32)
    q2, qb2 = np.concatenate([more[:300], q, more[300:]]), np.concatenate([more[:300, 0], qb, more[300:, 0]])
    off2 = np.concatenate([np.zeros(300, np.int64), off, np.full(212, off[-1], np.int64)])
    got = topk(q2, qb2, c, cb, K, 0, excl=(off2, ids_all))
    got = (got[0][300:333], got[1][300:333])
    assert all(np.array_equal(x, y) for x, y in zip(bits(got), bits(want)))


# ---------------------------------------------------------------- 6. end to end on tests/golden/tiny
def _tiny_model(mt, tmp_path):
    import reviews4rec_amd
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    kind = 'eval' if mt in ('deepconn', 'MF_dot') else 'e2e'
    meta, z = _fixture(mt, kind)
    root = materialise_tiny(tmp_path)
    train, test, val, hp = load_data(tiny_hp(mt, root), device=DEV)
    W = _weights(z, 'w/' if kind == 'eval' else 'best/')
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(W, strict=True)
    return hp, train, test, model.cuda().eval(), W


def _all_pairs(hp, test):
    """Every (user, item) pair in the loader's seven-slot layout, documents with nothing removed (data.py:240-246)."""
    U, I = hp['total_users'], hp['total_items']
    u, i = np.repeat(np.arange(U, dtype=np.int64), I), np.tile(np.arange(I, dtype=np.int64), U)
    none = np.full(len(u), -1, np.int64)
    fields = test._review_fields_host(u, i, none, none, none)
    return u, i, [torch.from_numpy(np.ascontiguousarray(f)) for f in fields] + [torch.from_numpy(u), torch.from_numpy(i)]


@pytest.mark.parametrize('mt', ['MF_dot', 'bias_only', 'deepconn'])
def test_catalogue_on_tiny_against_the_oracle(mt, tmp_path):
    import oracle
    from reviews4rec_amd import Catalogue
    from reviews4rec_amd import main as M
    hp, train, test, model, W = _tiny_model(mt, tmp_path)
    U, I, K = hp['total_users'], hp['total_items'], 5
    u, i, data = _all_pairs(hp, test)
    P64 = {k: (v.double() if v.is_floating_point() else v) for k, v in W.items()}
    with torch.no_grad():
        s64 = oracle.model_forward(P64, data, hp).numpy().astype(np.float64).reshape(U, I)
    cat = Catalogue(model, hp, train)
    eligible = sorted({int(r[1]) for r in train.data})
    assert cat.eligible.tolist() == eligible
    # (a) score_pairs against the float64 oracle forward
    got = cat.score_pairs(u, i).cpu().numpy().reshape(U, I)
    if mt == 'deepconn':
        tol = 1e-5 + 1e-5 * np.abs(s64)                       # the project's eval tolerance (test_gpu_models.py)
    else:
        D = hp['latent_size'] if mt == 'MF_dot' else 0
        q = W['user_embedding.weight'].numpy()[:U] if D else np.zeros((U, 0), np.float32)
        c = W['item_embedding.weight'].numpy()[:I] if D else np.zeros((I, 0), np.float32)
        qterms = np.abs(W['user_bias'].numpy()[:U]) + abs(float(W['global_bias']))
        tol = dot_bound(q, qterms, c, W['item_bias'].numpy()[:I], D)
    el = np.zeros(I, bool)
    el[eligible] = True
    assert (np.abs(got[:, el] - s64[:, el]) <= tol[:, el]).all(), float((np.abs(got[:, el] - s64[:, el]) / tol[:, el]).max())
    assert np.isneginf(got[:, ~el]).all()
    # (b) ... and against the package's own forward and the native engine's predict on the same pairs
    dev_data = [d.to(DEV) for d in data]
    engine = M.make_engine(dict(hp, engine='native'), model)
    with torch.no_grad():
        sliced = [engine.predict([d[a:a + 96] for d in dev_data], None)[0].clone() for a in range(0, U * I, 96)]
        for name, out in (('forward', model(dev_data)), ('predict', torch.cat(sliced))):
            mine = out.reshape(U, I).cpu().numpy().astype(np.float64)
            worst = float((np.abs(got[:, el] - mine[:, el]) / tol[:, el]).max())
            print('%s: score_pairs against %s, worst |difference| / tolerance = %.3f' % (mt, name, worst))
            assert (np.abs(got[:, el] - mine[:, el]) <= tol[:, el]).all(), (name, worst)        # the tolerance of (a)
    # (c), (d) the lists
    seen = {}
    for r in train.data:
        seen.setdefault(int(r[0]), set()).add(int(r[1]))
    users = np.arange(U, dtype=np.int64)
    for exclude in (True, False):
        ids, sc = cat.recommend(users, k=K, exclude_seen=exclude)
        assert ids.device.type == 'cuda' and ids.dtype == torch.int64 and sc.dtype == torch.float32
        ids, sc = ids.cpu().numpy(), sc.cpu().numpy()
        masked = np.where(el[None, :], s64, -np.inf)
        if exclude:
            for uu, items in seen.items():
                masked[uu, sorted(items)] = -np.inf
        demanded = check_lists(ids, sc, masked, np.where(np.isfinite(tol), tol, 0.0), K, '%s exclude=%s' % (mt, exclude))
        assert demanded >= 1, demanded
        assert np.isin(ids[ids >= 0], eligible).all()
        if exclude:
            assert not any(int(x) in seen.get(uu, ()) for uu in range(U) for x in ids[uu])
        # the list's scores are score_pairs' bits
        flat = ids.reshape(-1)
        again = cat.score_pairs(np.repeat(users, K)[flat >= 0], flat[flat >= 0]).cpu().numpy()
        assert np.array_equal(again.view(np.uint32), sc.reshape(-1)[flat >= 0].view(np.uint32))
    # candidates= overrides the default set
    few = Catalogue(model, hp, train, candidates=np.array(eligible[:3]))
    ids, _ = few.recommend(users[:4], k=K, exclude_seen=False)
    assert sorted(ids[0].cpu().tolist()) == [-1, -1] + eligible[:3]
    # ids may arrive as a device tensor
    a = cat.recommend(torch.from_numpy(users).to(DEV), k=K)
    b = cat.recommend(users.tolist(), k=K)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(cat.score_pairs(torch.from_numpy(u).to(DEV), torch.from_numpy(i).to(DEV)).cpu(),
                       torch.from_numpy(got.reshape(-1)))


# ---------------------------------------------------------------- 7. engines
def test_pending_mf_table_updates_are_flushed_first():
    """MFEngine's blocked sweeps leave table chunks behind until flush(): Catalogue(engine=engine) must see the tables a
    fresh Catalogue sees after an explicit flush."""
    from reviews4rec_amd import Catalogue
    from test_gpu_span import build, tiny_corpus
    corpus = tiny_corpus(seed=51)
    users = np.arange(300, dtype=np.int64)
    got = []
    for explicit in (False, True):
        hp, reader, model, engine = build('MF_dot', corpus)
        model.train()
        for step, (data, y) in enumerate(reader.iter()):
            engine.train_step(data, y, defer_sweep=True)
            if step == 4:
                break
        assert engine._pending() is not None                  # five steps into a period of eight: updates are pending
        if explicit:
            engine.flush()
            assert engine._pending() is None
        cat = Catalogue(model, hp, reader, engine=None if explicit else engine)
        assert engine._pending() is None
        ids, sc = cat.recommend(users, k=7)
        got.append((ids.cpu(), sc.cpu(), model.item_embedding.weight.detach().cpu().clone()))
    for a, b in zip(*got):
        assert torch.equal(a, b)
    assert (got[0][0] >= 0).all()


def test_a_recommend_pass_leaves_the_deepconn_training_state():
    """Train, recommend, continue == training never interrupted: weights, moments, offset, step_count, bit for bit (the
    fifth step's announced token batch is pending when the pass starts; dropout 0.5: a moved stream would show)."""
    from reviews4rec_amd import Catalogue
    from test_gpu_score_span import _snapshot
    from test_gpu_span import build, same, tiny_corpus
    corpus = tiny_corpus(seed=52)
    K = 5
    snaps = []
    for interrupt in (True, False):
        hp, reader, model, engine = build('deepconn', corpus, dropout=0.5)
        engine.conv_algo = 2                                  # the projection: the algorithm with token state, no probes
        model.train()
        desc = reader.span_descriptor()
        engine._span(desc, 0, K, True)
        if interrupt:
            cat = Catalogue(model, hp, reader, engine=engine, tower_batch=50)
            ids, sc = cat.recommend(np.arange(300), k=5)
            assert (ids[:, 0] >= 0).all() and torch.isfinite(sc[:, 0]).all() and model.training
        engine._span(desc, K, K, False)
        snaps.append(_snapshot(model, engine))
    same(snaps[0], snaps[1], 'interrupted against uninterrupted')
    assert snaps[0]['step'] == 2 * K


# ---------------------------------------------------------------- 8. main.main
@pytest.mark.parametrize('mt', ['MF_dot', 'deepconn'])
def test_main_writes_the_lists_of_the_trained_model(mt, tmp_path, monkeypatch):
    import reviews4rec_amd
    from reviews4rec_amd import Catalogue
    from reviews4rec_amd import main as M
    from reviews4rec_amd.data import load_data
    from test_tiny_eval import _fixture, _weights
    meta, z = _fixture(mt, 'e2e')
    root = materialise_tiny(tmp_path)

    def fixture_init(model):
        init = _weights(z, 'w/')
        model.load_state_dict({k: v.to(next(model.parameters()).device) for k, v in init.items()}, strict=True)

    monkeypatch.setattr(M, 'xavier_init', fixture_init)
    runs = {}
    for tag, extra in (('with', dict(recommend_k=3, recommend_path=str(tmp_path / 'lists.npz'))), ('without', {})):
        hp = tiny_hp(mt, root, log_file=str(tmp_path / ('log_' + tag)), model_path=str(tmp_path / ('model_' + tag)), **extra)
        before = set(os.listdir(str(tmp_path)))
        final = M.main(hp)
        runs[tag] = (final, torch.load(hp['model_path'], map_location='cpu'), set(os.listdir(str(tmp_path))) - before, hp)
    assert runs['with'][0] == runs['without'][0]                               # the metrics are what they were
    assert set(runs['with'][1]) == set(runs['without'][1])
    for k, v in runs['with'][1].items():
        assert torch.equal(v, runs['without'][1][k]), k
    assert runs['without'][2] == {'log_without', 'model_without'}, runs['without'][2]      # no file of lists
    assert 'lists.npz' in runs['with'][2]
    # the file's lists are Catalogue.recommend on the trained (best-on-validation) model
    hp = runs['with'][3]
    train, _, _, hp = load_data(hp, device=DEV)
    model = reviews4rec_amd.get_model_class(mt)(hp)
    model.load_state_dict(runs['with'][1])
    f = np.load(str(tmp_path / 'lists.npz'))
    users = np.array(sorted({int(r[0]) for r in train.data}), np.int64)
    assert np.array_equal(f['users'], users) and f['items'].shape == f['scores'].shape == (len(users), 3)
    ids, sc = Catalogue(model.cuda().eval(), hp, train).recommend(users, k=3)
    assert np.array_equal(f['items'], ids.cpu().numpy())
    assert np.array_equal(f['scores'].view(np.uint32), sc.cpu().numpy().view(np.uint32))
