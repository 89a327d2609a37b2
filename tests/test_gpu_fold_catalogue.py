"""``review_counterfactual`` and the ``fold`` attribute of the single-document catalogue classes on tests/golden/tiny at
input_length = 37 (recommend.py; include/r4r.h, "Document fold"): deepconn, deepconn++ and transnet++.

The search must equal a host loop of ``what_if`` calls with ``fold = True`` and a host arg-best (tower_fold_ref's
``candidates`` and ``better``), bit for bit, for every side and direction; budget 1 is the arg-best of
``leave_one_out``; ``k`` is a target written out by hand from ``recommend``; ``pair_batch``, the order of the pairs and
a pair alone change no bit.  ``leave_one_out`` with ``fold = True`` is held to the float64 reference and bound that
test_gpu_whatif_catalogue.py applies to the tower path, and with ``fold = False`` every call keeps its bits."""
import numpy as np
import pytest
import torch

import tower_fold_ref as R
from head_ref import U32, compare
from pair_grad_ref import pair_grad_ref
from test_gpu_pair_explain_catalogue import KIND, _float64_model
from test_gpu_phrases_catalogue import _catalogues
from test_gpu_whatif_catalogue import _grid, _side64, direct_conv, same_bits  # noqa: F401  (direct_conv: a fixture)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = 3


def _lens(cat, side, ids):
    pool = cat._phrase_side(side)[0]
    return [[int(pool.rev_off[pool.first[o] + s + 1] - pool.rev_off[pool.first[o] + s])
             for s in range(min(int(pool.first[o + 1] - pool.first[o]), 64))] for o in ids]


def _host_loop(cat, users, items, target, direction, side, budget):
    """The rule by ``what_if`` calls (``cat.fold`` is on): per step one call whose variants are every slot of both
    sides removed on top of the pair's masks; the host picks among the candidates."""
    n, T = len(users), int(cat.hp['input_length'])
    lens_u, lens_i = _lens(cat, 'user', users), _lens(cat, 'item', items)
    S_u, S_i = max(1, max(len(l) for l in lens_u)), max(1, max(len(l) for l in lens_i))
    d = 0 if direction == 'down' else 1
    mu, mi = [0] * n, [0] * n
    signed = lambda rows: torch.tensor([[x - (1 << 64) if x >= (1 << 63) else x for x in r] for r in rows], dtype=torch.int64)
    base = cat.what_if(users, items).base.cpu().numpy()
    order = np.full((n, budget), -1, np.int64)
    scores = np.repeat(base[:, None], budget + 1, 1)
    steps = np.zeros(n, np.int64)
    hit = np.array([R.crossed(base[p], target[p], d) for p in range(n)])
    done = hit.copy()
    for _ in range(budget):
        wu = [[mu[p] | (1 << s) for s in range(S_u)] + [mu[p]] * S_i for p in range(n)]
        wi = [[mi[p]] * S_u + [mi[p] | (1 << s) for s in range(S_i)] for p in range(n)]
        sc = cat.what_if(users, items, drop_user=signed(wu), drop_item=signed(wi)).scores.cpu().numpy()
        for p in range(n):
            if done[p]:
                continue
            best_s = best_c = None
            if side in ('user', 'both'):
                for s in R.candidates(lens_u[p], mu[p], (1 << 64) - 1, 64, T):
                    if R.better(best_s, best_c, sc[p, s], s, d):
                        best_s, best_c = sc[p, s], s
            if side in ('item', 'both'):
                for s in R.candidates(lens_i[p], mi[p], (1 << 64) - 1, 64, T):
                    if R.better(best_s, best_c, sc[p, S_u + s], R.ITEM + s, d):
                        best_s, best_c = sc[p, S_u + s], R.ITEM + s
            if best_c is None:
                done[p] = True
                continue
            if best_c < R.ITEM:
                mu[p] |= 1 << best_c
            else:
                mi[p] |= 1 << (best_c - R.ITEM)
            order[p, steps[p]] = best_c
            steps[p] += 1
            scores[p, steps[p]:] = best_s
            hit[p] = R.crossed(best_s, target[p], d)
            done[p] = hit[p] or steps[p] >= budget
    return order, scores, steps, hit


def _check(cf, want, target, budget):
    order, scores, steps, hit = want
    assert cf.order.cpu().numpy().tolist() == order.tolist()
    assert cf.scores.cpu().numpy().tobytes() == scores.astype(np.float32).tobytes()
    assert cf.steps.cpu().numpy().tolist() == steps.tolist() and cf.crossed.cpu().numpy().tolist() == hit.tolist()
    assert same_bits(cf.base, cf.scores[:, 0].contiguous())
    assert cf.target.cpu().numpy().tobytes() == np.asarray(target, np.float32).tobytes()
    for lo, removed in ((0, cf.removed_user), (R.ITEM, cf.removed_item)):
        for p in range(len(order)):
            mine = [int(c) - lo for c in order[p] if lo <= c < lo + R.ITEM]
            assert removed[p].tolist() == mine + [-1] * (budget - len(mine))


def _same_cf(a, b):
    return all(torch.equal(x, y) if x.dtype != torch.float32 else same_bits(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize('mt', ['deepconn', 'deepconn++', 'transnet++'])
def test_review_counterfactual_and_the_fold_attribute_on_tiny(mt, tmp_path, monkeypatch, direct_conv):
    import reviews4rec_amd
    cat, _, hp = _catalogues(mt, tmp_path, monkeypatch)
    T = int(hp['input_length'])
    assert T == 37 and cat.fold is False and type(cat).fold is False
    users, items = _grid(cat)
    n = len(users)
    drops = dict(drop_user=[[0] if c else [] for c in np.diff(cat._phrase_side('user')[0].first)[users]],
                 drop_item=torch.full((n, 1), 6, dtype=torch.int64))
    before = (cat.leave_one_out(users, items), cat.what_if(users, items, **drops))

    # ---- fold = True: leave_one_out within the tower path's float64 bound
    cat.fold = True
    loo = cat.leave_one_out(users, items)
    zu, pu, fc_u, own_u, row_u, _ = _side64(cat, 'user', users)
    zi, pi, fc_i, own_i, row_i, _ = _side64(cat, 'item', items)
    _, raw, qb, cb = _float64_model(cat, mt, own_u, own_i)
    pairs = [(p, -1, -1) for p in range(n)]
    pairs += [(p, s, -1) for p in range(n) for s in range(int(loo.live_user[p]))]
    pairs += [(p, -1, s) for p in range(n) for s in range(int(loo.live_item[p]))]
    u_idx = torch.tensor([row_u[(int(users[p]), su)] for p, su, _ in pairs])
    i_idx = torch.tensor([row_i[(int(items[p]), si)] for p, _, si in pairs])
    F = pu.shape[1]
    dz = lambda p, fc: (F + 1) * U32 * (p.abs() @ fc.weight.detach().abs().T + fc.bias.detach().abs())
    ref = pair_grad_ref(KIND[mt], zu, zi, u_idx, i_idx, {k: v.detach() for k, v in raw.items()}, fc_u.weight.detach(),
                        fc_i.weight.detach(), qb.detach(), None if cb is None else cb.detach(), dzu=dz(pu, fc_u),
                        dzi=dz(pi, fc_i))
    val, bound = ref['score'][0], ref['score'][1] + U32 * qb.detach()[u_idx].abs()
    got = torch.stack([loo.base[p] if su < 0 and si < 0 else (loo.without_user[p, su] if su >= 0 else loo.without_item[p, si])
                       for p, su, si in pairs])
    err = (got.detach().cpu().double() - val.cpu()).abs()
    print('%s: fold leave_one_out worst error / bound %.3f over %d scores'
          % (mt, float((err / bound.cpu().clamp(min=1e-300)).max()), len(pairs)))
    compare(mt + ' fold leave_one_out', got, val, bound)
    for a, b in zip(before[0][5:], loo[5:]):                 # live / reach: integers, the same either way
        assert torch.equal(a, b)

    # ---- the search against the host loop, every side and direction
    base = loo.base.cpu().numpy()
    deltas = np.abs(np.concatenate([loo.delta_user.cpu().numpy().ravel(), loo.delta_item.cpu().numpy().ravel()]))
    gap = float(np.median(deltas[deltas > 0])) / 2           # a target that a typical single removal can reach
    crossed = taken = 0
    for side in ('user', 'item', 'both'):
        for direction in ('down', 'up'):
            target = (base + (-gap if direction == 'down' else gap)).astype(np.float32)
            target[0], target[1], target[2] = np.nan, np.inf, -np.inf
            cf = cat.review_counterfactual(users, items, target=torch.from_numpy(target), direction=direction, side=side,
                                           budget=B)
            assert isinstance(cf, reviews4rec_amd.Counterfactual) and tuple(cf.order.shape) == (n, B)
            want = _host_loop(cat, users, items, target, direction, side, B)
            _check(cf, want, target, B)
            crossed, taken = crossed + int(want[3].sum()), taken + int(want[2].sum())
    print('%s: %d steps taken, %d searches crossed' % (mt, taken, crossed))
    assert taken > n and crossed > 0

    # ---- budget 1 is leave_one_out's arg-best
    never = np.full(n, -np.inf, np.float32)
    one = cat.review_counterfactual(users, items, target=torch.from_numpy(never), side='both', budget=1)
    wu, wi = loo.without_user.cpu().numpy(), loo.without_item.cpu().numpy()
    lens_u, lens_i = _lens(cat, 'user', users), _lens(cat, 'item', items)
    for p in range(n):
        best_s = best_c = None
        for s in R.candidates(lens_u[p], 0, (1 << 64) - 1, 64, T):
            if R.better(best_s, best_c, wu[p, s], s, 0):
                best_s, best_c = wu[p, s], s
        for s in R.candidates(lens_i[p], 0, (1 << 64) - 1, 64, T):
            if R.better(best_s, best_c, wi[p, s], R.ITEM + s, 0):
                best_s, best_c = wi[p, s], R.ITEM + s
        assert int(one.order[p, 0]) == (-1 if best_c is None else best_c)
        if best_c is not None:
            assert np.float32(one.scores[p, 1].item()).tobytes() == np.float32(best_s).tobytes()

    # ---- k: the target written out by hand from recommend
    k = 2
    real = users < cat.n_users                               # (the owner without a review is no user of the catalogue)
    users, items, n = users[real], items[real], int(real.sum())
    lists, scores = cat.recommend(torch.from_numpy(users), k + 1)
    hand = np.full(n, -np.inf, np.float32)
    for p in range(n):
        other = [(int(it), float(sc)) for it, sc in zip(lists[p].tolist(), scores[p].tolist()) if it != int(items[p]) and it >= 0]
        if len(other) >= k:
            hand[p] = np.float32(other[k - 1][1])
    by_k = cat.review_counterfactual(users, items, k=k, side='item', budget=2)
    assert by_k.target.cpu().numpy().tobytes() == hand.tobytes()
    whole = cat.review_counterfactual(users, items, target=torch.from_numpy(hand), side='item', budget=2)
    assert _same_cf(by_k, whole)

    # ---- pair_batch, the order of the pairs, a pair alone, no pair
    for pb in (1, 3, 8192):
        cat.pair_batch = pb
        assert _same_cf(cat.review_counterfactual(users, items, target=torch.from_numpy(hand), side='item', budget=2), whole), pb
    perm = np.random.RandomState(0).permutation(n)
    got = cat.review_counterfactual(users[perm], items[perm], target=torch.from_numpy(hand[perm]), side='item', budget=2)
    assert _same_cf(got, [t[torch.from_numpy(perm).to(t.device)] for t in whole])
    p = int(np.argmax(whole.steps.cpu().numpy()))
    alone = cat.review_counterfactual(users[p:p + 1], items[p:p + 1], target=float(hand[p]), side='item', budget=2)
    assert _same_cf(alone, [t[p:p + 1] for t in whole])
    none = cat.review_counterfactual([], [], target=1.0, budget=4)
    assert tuple(none.order.shape) == (0, 4) and tuple(none.scores.shape) == (0, 5)

    # ---- fold = False: every call keeps the bits it had
    users, items = _grid(cat)
    with_fold = cat.what_if(users, items, **drops)
    cat.fold = False
    after = (cat.leave_one_out(users, items), cat.what_if(users, items, **drops))
    for a, b in zip(before[0], after[0]):
        assert same_bits(a, b) if a.dtype == torch.float32 else torch.equal(a, b)
    assert same_bits(before[1].scores, after[1].scores) and same_bits(before[1].base, after[1].base)
    assert float((with_fold.scores - after[1].scores).abs().max()) < 1e-4      # the same numbers by another fp32 chain
