"""r4r_textcnn_phrases on the device (include/r4r.h, "Phrase explanations"; csrc/phrases.hip) against phrases_ref, the
sequential np.float32 loop in ascending f of tests/phrases_ref.py, over synthetic pooled / argmax:

    F in {1, 63, 64, 65, 100, 112}  x  T in {1, 3, 40}  x  N in {1, 5, 257}  x  K in {1, 3, F}

(K = 3 at F = 1 is outside 1 .. F: the entry point refuses it, tests/test_phrases_host.py; there K is {1}.)  Without
weights everything is exact: positions, score BITS, filter counts, n_windows, tokens.  With weights a listed score is
held to the fma chain's own bound against the float64 sum, (c + 1) 2^-24 sum |w_f pooled_f| over its c filters, the list
at K = F must be the host sort of the kernel's own score bits, and -- beyond the bound -- the first rows must carry the
bits of the exactly rounded chain (phrases_ref.fma32).  A shape's inputs and references are computed once per (F, T)
and shared by the tests of that shape."""
import functools

import numpy as np
import pytest
import torch

from phrases_ref import bits, phrases_ref, tokens_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
FS, TS, NS = (1, 63, 64, 65, 100, 112), (1, 3, 40), (1, 5, 257)
N_MAX = max(NS)


def ks(F):
    return sorted({1, min(3, F), F})


@functools.lru_cache(maxsize=None)
def case(F, T):
    """The inputs of one shape, 257 rows (a smaller N takes the first rows), and the unweighted reference at K = F."""
    rng = np.random.default_rng(1000 * F + T)
    pooled = rng.random((N_MAX, F)).astype(np.float32) * 3
    pooled[::2] = rng.integers(0, 9, size=pooled[::2].shape).astype(np.float32) / 8   # exact sums: windows that tie
    argmax = rng.integers(-1, T + 3, size=(N_MAX, F)).astype(np.int32)                # -1 and T + 2: dead
    argmax[pooled == 0] = -1                                                          # what the conv writes there
    idx = rng.integers(0, 50, size=(N_MAX, T)).astype(np.int64)                       # (0: the pad word is a word too)
    shared = rng.standard_normal(F).astype(np.float32)                                # signs mixed
    per_row = rng.standard_normal((N_MAX, F)).astype(np.float32)
    ref = phrases_ref(pooled, argmax, None, T, F)
    tok = tokens_ref(ref[0], idx, T)
    for a in (pooled, argmax, idx, shared, per_row, tok) + ref:
        a.setflags(write=False)
    return dict(pooled=pooled, argmax=argmax, idx=idx, shared=shared, per_row=per_row, ref=ref, tok=tok)


def device(a):
    return None if a is None else torch.from_numpy(np.array(a)).to(DEV)        # (a copy: the shared inputs are read-only)


def run(pooled, argmax, K, T, wt=None, idx=None):
    """ops.textcnn_phrases over host arrays -> host arrays (positions, scores, filters, tokens or None, windows)."""
    from reviews4rec_amd import ops
    out = ops.textcnn_phrases(device(pooled), device(argmax), K, T, weights=device(wt), idx=device(idx))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in out)


def raw(pooled, argmax, K, T, wt=None, idx=None, want=('pos', 'score', 'filt', 'tok', 'win')):
    """The entry point itself, outputs pre-filled with -7, those not in ``want`` passed as NULL -> dict of host arrays."""
    from reviews4rec_amd import _lib
    from reviews4rec_amd._lib import ptr
    N, F = pooled.shape
    p, a, w, d = device(pooled), device(argmax), device(wt), device(idx)
    shapes = dict(pos=((N, K), torch.int32), score=((N, K), torch.float32), filt=((N, K), torch.int32),
                  tok=((N, K, 3), torch.int64), win=((N,), torch.int32))
    out = {k: torch.full(s, -7, dtype=t, device=DEV) for k, (s, t) in shapes.items() if k in want}
    _lib.call('r4r_textcnn_phrases', ptr(p), ptr(a), ptr(w), 0 if wt is None or wt.ndim == 1 else F, ptr(d), N, T, F, K,
              *[ptr(out.get(k)) for k in ('pos', 'score', 'filt', 'tok', 'win')])
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, what):
    """Five outputs, bit for bit."""
    for name, g, w in zip(('positions', 'scores', 'filters', 'tokens', 'windows'), got, want):
        if name == 'scores':
            g, w = bits(g), bits(w)
        assert g.dtype == w.dtype and np.array_equal(g, w), (what, name)


# ---------------------------------------------------------------- without weights: exact
@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('F', FS)
def test_activation_mass_is_the_reference_bit_for_bit(F, T):
    c = case(F, T)
    pos, score, filt, win = c['ref']
    assert F == 1 or win.max() > 1                          # the shape has rows with several windows
    for N in NS:
        for K in ks(F):
            got = run(c['pooled'][:N], c['argmax'][:N], K, T, idx=c['idx'][:N])
            want = (pos[:N, :K], score[:N, :K], filt[:N, :K], c['tok'][:N, :K], win[:N])
            same(got, want, (F, T, N, K))


# ---------------------------------------------------------------- with weights: the fma chain's bound, the kernel's own order
def float64_sums(pooled, argmax, wt, pos):
    """Per listed window of ``pos`` [N, K]: (float64 sum of w_f pooled_f, sum of |w_f pooled_f|, c) over its filters."""
    member = (argmax[:, None, :] == pos[:, :, None]) & (pos[:, :, None] >= 0)          # [N, K, F]
    prod = (np.broadcast_to(wt, pooled.shape).astype(np.float64) * pooled.astype(np.float64))[:, None, :]
    return (prod * member).sum(2), (np.abs(prod) * member).sum(2), member.sum(2)


@pytest.mark.parametrize('form', ['shared', 'per_row'])
@pytest.mark.parametrize('T', TS)
@pytest.mark.parametrize('F', FS)
def test_weighted_scores_meet_the_chain_s_bound_and_the_list_is_the_sort_of_its_own_bits(F, T, form):
    c = case(F, T)
    ref_pos, _, ref_filt, ref_win = c['ref']                 # which windows exist does not depend on the weights
    for N in NS:
        pooled, argmax, idx = c['pooled'][:N], c['argmax'][:N], c['idx'][:N]
        wt = c['shared'] if form == 'shared' else c['per_row'][:N]
        pos, score, filt, tok, win = run(pooled, argmax, F, T, wt=wt, idx=idx)
        assert np.array_equal(win, ref_win[:N])
        s64, mass, count = float64_sums(pooled, argmax, wt, pos)
        listed = pos >= 0
        assert np.array_equal(listed.sum(1), win) and np.array_equal(listed, np.arange(F)[None, :] < win[:, None])
        assert np.array_equal(filt, count) and (filt[listed] > 0).all()
        err, bound = np.abs(score.astype(np.float64) - s64), (count + 1) * 2.0 ** -24 * mass
        if listed.any() and N == N_MAX:
            print('phrases F=%d T=%d %s: worst |score - float64| / bound = %.3f'
                  % (F, T, form, float((err[listed] / np.maximum(bound[listed], 1e-300)).max())))
        assert (err[listed] <= bound[listed]).all(), (N, float((err - bound)[listed].max()))
        assert (bits(score)[~listed] == 0).all() and (filt[~listed] == 0).all()
        for n in range(N):
            w = int(win[n])
            assert sorted(pos[n, :w].tolist()) == sorted(ref_pos[n, :w].tolist())      # every window once
            order = np.lexsort((pos[n, :w], -score[n, :w].astype(np.float64)))
            assert np.array_equal(order, np.arange(w)), (N, n)                          # score descending, then position
        assert np.array_equal(tok, tokens_ref(pos, idx, T))
        # a shorter list is the head of this one
        for K in ks(F)[:-1]:
            same(run(pooled, argmax, K, T, wt=wt, idx=idx), (pos[:, :K], score[:, :K], filt[:, :K], tok[:, :K], win), (N, K))
        if N == 5:                                            # the exactly rounded chain, a few rows
            want = phrases_ref(pooled, argmax, wt, T, F)
            same((pos, score, filt, tok, win), want[:3] + (tokens_ref(want[0], idx, T), want[3]), 'fma bits')


# ---------------------------------------------------------------- edge rows
def edge_rows(F, T):
    """(pooled, argmax, what each row is).  Dead filters keep a nonzero pooled value: being dead is argmax's say."""
    rows, names = [], []

    def row(name, arg, val=None):
        a = np.full(F, -1, np.int32)
        a[:len(arg)] = arg
        rows.append((np.full(F, 0.5, np.float32) if val is None else val, a))
        names.append(name)

    row('all on one window', np.full(F, 7 % (T + 2)))
    row('F distinct windows', np.arange(F), (np.arange(F, dtype=np.float32) * 7 % 13 + 1) / 4)   # needs T + 2 >= F
    row('all dead', np.resize(np.array([-1, -7, T + 2, 1 << 30, -(1 << 31), T + 3], np.int64), F).astype(np.int32))
    row('the first and the last positions', np.resize(np.array([0, 1, T, T + 1]), min(F, 4)),
        np.array([1, 2, 3, 4] * 28, np.float32)[:F])
    row('equal score bits', np.array([9, 4, 4, 9, 2][:F]), np.array([0.5, 0.25, 0.25, 0.5, 0.5] + [1.0] * 107, np.float32)[:F])
    if F > 67:
        a = np.full(F, -1, np.int32)
        a[3] = a[67] = 5                                      # the two filters of lane 3
        a[63] = a[64] = 6                                     # the last lane's first filter, the first lane's second
        a[0] = a[F - 1] = 11                                  # the first and the last filter
        row('pairs across the halves', a, (np.arange(F, dtype=np.float32) + 1) / 16)
    return np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]), names


@pytest.mark.parametrize('F', FS)
def test_edge_rows(F):
    T = 120                                                   # T + 2 >= 112: room for F distinct windows
    pooled, argmax, names = edge_rows(F, T)
    idx = np.arange(1, T + 1, dtype=np.int64)[None, :].repeat(len(names), 0) * 3
    full = phrases_ref(pooled, argmax, None, T, F)
    for K in ks(F):
        got = run(pooled, argmax, K, T, idx=idx)
        same(got, (full[0][:, :K], full[1][:, :K], full[2][:, :K], tokens_ref(full[0][:, :K], idx, T), full[3]), (F, K))
    pos, score, filt, tok, win = run(pooled, argmax, F, T, idx=idx)
    at = {n: i for i, n in enumerate(names)}
    i = at['all on one window']
    assert win[i] == 1 and pos[i, 0] == 7 and filt[i, 0] == F and score[i, 0] == np.float32(0.5) * F
    assert (pos[i, 1:] == -1).all() and (tok[i, 1:] == -1).all()
    i = at['F distinct windows']
    assert win[i] == F and sorted(pos[i].tolist()) == list(range(F)) and (filt[i] == 1).all()
    i = at['all dead']
    assert win[i] == 0 and (pos[i] == -1).all() and (bits(score[i]) == 0).all() and (filt[i] == 0).all() and (tok[i] == -1).all()
    i = at['the first and the last positions']
    by_pos = {int(p): tok[i, k].tolist() for k, p in enumerate(pos[i]) if p >= 0}
    assert by_pos[0] == [-1, -1, 3]
    if F >= 4:
        assert by_pos[1] == [-1, 3, 6] and by_pos[T] == [3 * (T - 1), 3 * T, -1] and by_pos[T + 1] == [3 * T, -1, -1]
    i = at['equal score bits']
    if F >= 5:
        assert pos[i, :3].tolist() == [9, 2, 4] and bits(score[i, 1]) == bits(score[i, 2]) and filt[i, :3].tolist() == [2, 1, 2]
    if F > 67:
        i = at['pairs across the halves']
        got = {int(p): (float(s), int(f)) for p, s, f in zip(pos[i], score[i], filt[i]) if p >= 0}
        assert got == {5: ((4 + 68) / 16, 2), 6: ((64 + 65) / 16, 2), 11: ((1 + F) / 16, 2)}


# ---------------------------------------------------------------- a row's outputs depend on that row only
@pytest.mark.parametrize('form', [None, 'per_row'])
@pytest.mark.parametrize('F, T', [(112, 40), (65, 3), (64, 1)])
def test_a_row_s_outputs_do_not_depend_on_the_call(F, T, form):
    c = case(F, T)
    N = 257
    pooled, argmax, idx = c['pooled'], c['argmax'], c['idx']
    wt = None if form is None else c['per_row']
    whole = raw(pooled, argmax, F, T, wt=wt, idx=idx)
    names = ('pos', 'score', 'filt', 'tok', 'win')
    eq = lambda a, b: np.array_equal(a.view(np.uint32) if a.dtype == np.float32 else a, b.view(np.uint32) if b.dtype == np.float32 else b)
    # permuted rows
    perm = np.random.default_rng(5).permutation(N)
    got = raw(pooled[perm], argmax[perm], F, T, wt=None if wt is None else wt[perm], idx=idx[perm])
    assert all(eq(got[k], whole[k][perm]) for k in names)
    # split calls: one row, five rows, the rest
    for a, b in ((0, 1), (1, 6), (6, N)):
        got = raw(pooled[a:b], argmax[a:b], F, T, wt=None if wt is None else wt[a:b], idx=idx[a:b])
        assert all(eq(got[k], whole[k][a:b]) for k in names), (a, b)
    # another K: the head of the list
    for K in ks(F)[:-1]:
        got = raw(pooled, argmax, K, T, wt=wt, idx=idx)
        assert all(eq(got[k], whole[k][:, :K]) for k in names[:4]) and eq(got['win'], whole['win']), K
    # NULL outputs: each output alone, and without the documents
    for k in names:
        got = raw(pooled, argmax, F, T, wt=wt, idx=idx if k == 'tok' else None, want=(k,))
        assert list(got) == [k] and eq(got[k], whole[k]), k
    got = raw(pooled, argmax, F, T, wt=wt, idx=None, want=('pos', 'score'))
    assert eq(got['pos'], whole['pos']) and eq(got['score'], whole['score'])


def test_the_wrapper_checks_its_arguments():
    from reviews4rec_amd import ops
    c = case(64, 3)
    p, a = device(c['pooled'][:5]), device(c['argmax'][:5])
    for bad in (dict(weights=torch.zeros(63, device=DEV)), dict(weights=torch.zeros(4, 64, device=DEV)),
                dict(idx=torch.zeros(5, 4, dtype=torch.int64, device=DEV)),
                dict(idx=torch.zeros(5, 3, dtype=torch.int32, device=DEV))):
        with pytest.raises(RuntimeError):
            ops.textcnn_phrases(p, a, 3, 3, **bad)
    for kw in (dict(pooled=p.cpu()), dict(argmax=a.to(torch.int64)), dict(argmax=a[:4]), dict(k=0), dict(k=65)):
        args = dict(pooled=p, argmax=a, k=3, T=3)
        args.update(kw)
        with pytest.raises(RuntimeError):
            ops.textcnn_phrases(**args)
    out = ops.textcnn_phrases(p, a, 3, 3)
    assert out[3] is None and out[0].shape == (5, 3) and out[4].dtype == torch.int32
    empty = ops.textcnn_phrases(p[:0], a[:0], 3, 3, idx=torch.zeros(0, 3, dtype=torch.int64, device=DEV))
    assert empty[0].shape == (0, 3) and empty[3].shape == (0, 3, 3)
