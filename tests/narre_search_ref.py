"""The greedy rule of NARRE's counterfactual search (include/r4r.h, "NARRE counterfactual search";
csrc/narre_search.hip) on the host, over ANY scorer of (pair, user mask, item mask) variants: narre_whatif_ref's float64
``whatif_ref`` with its per-element bounds, its float32 numpy evaluation in another summation order, or -- in the GPU
tests -- the existing kernel ``ops.narre_whatif``, whose bits the search must give.  Also the seeded searches the host
and the GPU tests share.  No kernel of the project and no GPU code lives here.

The rule, per pair: the masks start at ``start``; score 0 is the score under them.  While the comparison against the
target does not hold (strict float compares; NaN never holds) and fewer than ``budget`` removals were made, the
candidates are the slots set in ``cand``, not yet removed and currently SELECTED (among the first R clear slots of their
side), numbered c = slot (user) / 64 + slot (item); each is scored with that one more bit; the lowest (down) or highest
(up) score is taken, walking c ascending and replacing the best only by a strictly better one (a number over a NaN), so
ties go to the lowest c.  No candidate left ends the search."""
import numpy as np
import torch

from head_ref import _gen
from narre_whatif_ref import ARGS, N_I, N_U, whatif_f32, whatif_inputs, whatif_ref

ITEM = 64
M64 = (1 << 64) - 1
INF, NAN = float('inf'), float('nan')


def as_i64(v):
    v &= M64
    return v - (1 << 64) if v >= (1 << 63) else v


def selected_bits(mask, S, R):
    """The first R clear slots of 0 .. S - 1 under ``mask`` (a Python int), as a bit set."""
    out = n = 0
    for s in range(S):
        if n == R:
            break
        if not (mask >> s) & 1:
            out |= 1 << s
            n += 1
    return out


def candidates(mu, mi, may_u, may_i, shape):
    """-> [(c, mask_u', mask_i')] in ascending c: the slots of ``may_*`` that are not removed and currently selected."""
    S_u, R_u, S_i, R_i = shape
    out = []
    left = selected_bits(mu, S_u, R_u) & may_u & ~mu
    out += [(s, mu | (1 << s), mi) for s in range(S_u) if (left >> s) & 1]
    left = selected_bits(mi, S_i, R_i) & may_i & ~mi
    out += [(ITEM + s, mu, mi | (1 << s)) for s in range(S_i) if (left >> s) & 1]
    return out


def better(s, best, up):
    """Does score ``s`` replace ``best`` (None: nothing yet)?  The kernel's rule, in float compares."""
    if best is None:
        return True
    if best != best:
        return s == s
    return s > best if up else s < best


def holds(s, target, up):
    return bool(s > target) if up else bool(s < target)


def greedy(score_fn, shape, u_idx, i_idx, start_u, start_i, cand_u, cand_i, target, direction, budget, follow=None):
    """The search of every pair, in lockstep: one ``score_fn(u, i, mask_u, mask_i)`` call (int64 tensors [N] -> scores
    [N], or (scores, bounds)) for the start masks and one per step over all pairs' candidates.  ``start_*`` / ``cand_*``:
    int64 [n_p] tensors or None.  ``follow``: int [n_p, B] -- take THAT step instead of the best (a replay of another
    search; the step must be a candidate), until its -1.
    -> dict(order int32 [n_p, B], scores [n_p, B + 1] in the scorer's dtype, steps int32, crossed int32, mask_u, mask_i
    (the final masks, Python ints) and trace: per taken step (pair, step, c, score, bound, best_c, best score, best
    bound, runner-up score or None, number of candidates))."""
    S_u, R_u, S_i, R_i = shape
    up = direction == 1
    n = int(u_idx.numel())
    ints = lambda t: [0] * n if t is None else [int(v) & M64 for v in t.tolist()]
    all_u, all_i = (1 << S_u) - 1, (1 << S_i) - 1
    mu, mi = [m & all_u for m in ints(start_u)], [m & all_i for m in ints(start_i)]
    may_u = [c & all_u & ~m for c, m in zip(ints(cand_u), mu)]
    may_i = [c & all_i & ~m for c, m in zip(ints(cand_i), mi)]
    tgt = [float(v) for v in torch.as_tensor(target).to(torch.float64).tolist()]
    t64 = lambda masks: torch.tensor([as_i64(m) for m in masks], dtype=torch.int64)

    def run(us, is_, mus, mis):
        got = score_fn(torch.tensor(us, dtype=torch.int64), torch.tensor(is_, dtype=torch.int64), t64(mus), t64(mis))
        sc, bd = got if isinstance(got, tuple) else (got, None)
        sc = np.asarray(torch.as_tensor(sc).detach().cpu().numpy()).reshape(-1)
        bd = None if bd is None else np.asarray(torch.as_tensor(bd).detach().cpu().numpy()).reshape(-1)
        return sc, bd
    ul, il = u_idx.tolist(), i_idx.tolist()
    base, _ = run(ul, il, mu, mi) if n else (np.zeros(0, np.float32), None)
    scores = np.zeros((n, budget + 1), base.dtype)
    order = np.full((n, budget), -1, np.int32)
    steps, crossed = np.zeros(n, np.int32), np.zeros(n, np.int32)
    scores[:, 0] = base
    now = [base[p].item() for p in range(n)]
    done = [holds(now[p], tgt[p], up) for p in range(n)]
    crossed[:] = done
    trace = []
    for t in range(budget):
        flat, spans = [], {}
        for p in range(n):
            if done[p] or (follow is not None and int(follow[p][t]) < 0):
                done[p] = True
                continue
            cs = candidates(mu[p], mi[p], may_u[p], may_i[p], shape)
            if not cs:
                done[p] = True
                continue
            spans[p] = (len(flat), cs)
            flat += [(ul[p], il[p], a, b) for _, a, b in cs]
        if not flat:
            break
        sc, bd = run(*zip(*flat))
        for p, (at, cs) in spans.items():
            best = best_k = run_up = None
            for k in range(len(cs)):
                s = sc[at + k].item()
                if better(s, best, up):
                    best, best_k, run_up = s, k, best
                elif better(s, run_up, up):
                    run_up = s
            take = best_k
            if follow is not None:
                take = [c for c, _, _ in cs].index(int(follow[p][t]))      # ValueError: the step was no candidate
            c, mu[p], mi[p] = cs[take]
            now[p] = sc[at + take].item()
            order[p, t], scores[p, t + 1], steps[p] = c, sc[at + take], t + 1
            bound = lambda k: None if bd is None else float(bd[at + k])
            trace.append((p, t, c, now[p], bound(take), cs[best_k][0], best, bound(best_k), run_up, len(cs)))
            if holds(now[p], tgt[p], up):
                done[p], crossed[p] = True, 1
    for p in range(n):
        scores[p, steps[p] + 1:] = scores[p, steps[p]]
    return dict(order=order, scores=scores, steps=steps, crossed=crossed, mask_u=mu, mask_i=mi, trace=trace)


# ------------------------------------------------------------------------------------------------------------ the scorers
def scorer64(d):
    """``whatif_ref`` (float64, with bounds; it asserts the ReLU margins of every variant it scores)."""
    def fn(u, i, mu, mi):
        ref = whatif_ref(d['user'], d['item'], u, i, mu[:, None], mi[:, None], d['W1'], d['b1'], d['w'], d['q_bias'],
                         d['c_bias'])
        return ref['score'][0][:, 0], ref['score'][1][:, 0]
    return fn


def scorer32(d):
    """``whatif_f32``: numpy float32 in another summation order."""
    def fn(u, i, mu, mi):
        return whatif_f32(d['user'], d['item'], u, i, mu[:, None], mi[:, None], d['W1'], d['b1'], d['w'], d['q_bias'],
                          d['c_bias'])[:, 0]
    return fn


# ===================================================================================================== cases and inputs
TARGETS = (-INF, NAN, 0.0, -1.0, 1.0, -2.0, 2.0, 0.5, -0.5, 3.0, -3.0, INF)


def search_inputs(R_u, S_u, R_i, S_i, L, n_p=N_U * N_I, seed=0, biases=True, own=True):
    """A case's inputs: ``whatif_inputs``' sides, head and pair walk (3 users x 4 items, the twelve pairs first), and per
    PAIR (not per place in the call, so a repeated pair repeats its search) the start masks, the candidate masks and
    the target:
      start   pair k % 4 == 1: slot 0 of the user, and a bit >= S;  == 2: slot 1 (or 0) of the item and bit 63;
              == 3: the item's slots 0 and S - 1
      cand    all bits (bits >= S and start's own among them); pair 4: no candidate at all; pair 5: the user's alone;
              pair 6: the item's alone; pair 7: one slot a side; pair 8: every second slot
      target  TARGETS walked by the pair's number."""
    d = whatif_inputs(R_u, S_u, R_i, S_i, L, 1, n_p, seed, biases=biases, own=own)
    d.pop('drop_u'), d.pop('drop_i')
    start_u, start_i, cand_u, cand_i, target = [], [], [], [], []
    for k in range(N_U * N_I):
        su = si = 0
        if k % 4 == 1:
            su = 1 | (1 << min(S_u, 63))
        elif k % 4 == 2:
            si = (1 << min(1, S_i - 1)) | (1 << 63)
        elif k % 4 == 3:
            si = 1 | (1 << (S_i - 1))
        cu = ci = M64
        if k == 4:
            cu = ci = 0
        elif k == 5:
            ci = 0
        elif k == 6:
            cu = 0
        elif k == 7:
            cu, ci = 1 << (S_u // 2), 1 << (S_i // 2)
        elif k == 8:
            cu = ci = 0x5555555555555555
        start_u.append(as_i64(su)), start_i.append(as_i64(si)), cand_u.append(as_i64(cu)), cand_i.append(as_i64(ci))
        target.append(TARGETS[k % len(TARGETS)])
    pair = d['u_idx'] * N_I + d['i_idx']
    pick = lambda vals, dt: torch.tensor(vals, dtype=dt)[pair].contiguous()
    d.update(start_u=pick(start_u, torch.int64), start_i=pick(start_i, torch.int64), cand_u=pick(cand_u, torch.int64),
             cand_i=pick(cand_i, torch.int64), target=pick(target, torch.float32), shape=(S_u, R_u, S_i, R_i))
    return d


MASKS = ('start_u', 'start_i', 'cand_u', 'cand_i')


def search_of(score_fn, d, direction, budget, follow=None, **over):
    a = dict({k: d[k] for k in ('u_idx', 'i_idx', 'target') + MASKS}, **over)
    return greedy(score_fn, d['shape'], a['u_idx'], a['i_idx'], a['start_u'], a['start_i'], a['cand_u'], a['cand_i'],
                  a['target'], direction, budget, follow=follow)


# (R_u, S_u, R_i, S_i, L, budget, n_p): the issue's (R, S), L, budget and n_p values, each at least once, the two sides
# differing once.  One slot; slide-in at R = 1; one staged group; two and ten spare slots; ragged; the limit (128
# candidates, 8 MFMA groups).
CASES = [
    (1, 1, 1, 1, 1, 1, 1), (1, 3, 1, 3, 16, 2, 5), (5, 5, 5, 5, 17, 5, 257), (10, 12, 10, 12, 33, 10, 5),
    (10, 20, 10, 20, 64, 2, 257), (10, 20, 10, 20, 16, 64, 5), (33, 40, 33, 40, 17, 33, 5), (64, 64, 64, 64, 64, 2, 5),
    (64, 64, 64, 64, 16, 64, 1), (5, 5, 10, 12, 33, 64, 5), (10, 12, 10, 12, 1, 10, 257), (33, 40, 33, 40, 64, 1, 1),
]
# the cases that also go against float64 (the float64 scorer asserts the ReLU margin of EVERY candidate it scores, so
# the seed is one at which they all hold: ``find_seed`` of narre_whatif_ref is how they are found)
F64_CASES = [(1, 3, 1, 3, 16, 2, 5), (5, 5, 5, 5, 17, 5, 257), (10, 12, 10, 12, 33, 10, 5), (10, 20, 10, 20, 64, 2, 257),
             (5, 5, 10, 12, 33, 64, 5), (33, 40, 33, 40, 17, 33, 5)]
F64_SEEDS = {(10, 12, 10, 12, 33, 10, 5): 1, (10, 20, 10, 20, 64, 2, 257): 1, (33, 40, 33, 40, 17, 33, 5): 52,
             (64, 64, 64, 64, 64, 2, 5): 9}      # (the last: the owner pass's margins, as narre_whatif_ref's SEEDS)


def case_inputs(case, n_p=None, **how):
    R_u, S_u, R_i, S_i, L, _, n = case
    return search_inputs(R_u, S_u, R_i, S_i, L, n if n_p is None else n_p, F64_SEEDS.get(case, 0), **how)


def agreement(d, direction, budget):
    """The float64 search of a case's twelve pairs, and the float32 numpy scorer walked along it -> (float64 result,
    steps taken, steps at which float32's best is float64's)."""
    r64 = search_of(scorer64(d), d, direction, budget)
    r32 = search_of(scorer32(d), d, direction, budget, follow=r64['order'])
    same = sum(1 for t in r32['trace'] if t[2] == t[5])
    return r64, len(r32['trace']), same
