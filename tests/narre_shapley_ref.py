"""NARRE Shapley values (include/r4r.h, "NARRE Shapley values"; csrc/narre_shapley.hip) on the host, in numpy float64:
the coefficient table, the coalition form ``shapley_from_values``, an independent brute force by the permutation
definition, the mask-from-coalition rule, the per-rounding bound of the kernel's accumulation rule, a float64 scorer of
every coalition and the seeded cases the host and the GPU tests share.  No kernel of the project and no GPU code lives
here.

The bound, in tests/head_ref.py's way, for phi_t of a pair of n players against ``shapley_from_values`` applied to the
SAME fp32 values v(c).  With d_c = v(c) - v(2^n - 1) and M_t = sum_c |coef_t(c)| |d_c| in float64:
  the weight a_k is formed in float64 and rounded to fp32 once                  2^-24 M_t  (+ 2^-52 M_t for the float64 step)
  d_c is a float64 difference of two floats                                     2^-53 M_t
  a lane chains at most 64 fma of a chunk's coalitions, one rounding each       64 2^-53 M_t
  the 16 lane sums meet in four butterfly additions                             4 2^-53 M_t
  the chunk sums are chained, one addition a chunk                              chunks 2^-53 M_t
  the total is rounded to fp32 once                                             2^-24 |phi_t| <= 2^-24 M_t  (+ 2^-149)
  the float64 reference sums 2^n terms in numpy's order                         2^n 2^-53 M_t
so   |kernel - reference| <= (2 2^-24 + (72 + chunks + 2^n) 2^-53) M_t + 2^-149."""
import itertools
import math
from fractions import Fraction

import numpy as np
import torch

from narre_search_ref import as_i64
from narre_whatif_ref import N_I, N_U, select, whatif_inputs

MAX_PLAYERS = 16
CHUNK_LOG = 10
U32, U64 = 2.0 ** -24, 2.0 ** -53
M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------------ the coefficients
def exact_weights(n):
    """a_k = (k - 1)! (n - k)! / n! as Fractions, k = 0 .. n + 1 (0 at both ends)."""
    f = math.factorial
    return [Fraction(0)] + [Fraction(f(k - 1) * f(n - k), f(n)) for k in range(1, n + 1)] + [Fraction(0)]


def weights(n):
    return np.array([float(a) for a in exact_weights(n)], dtype=np.float64)


def coefficients(n, a=None):
    """float64 [n, 2^n]: coef_t(c) = a_k for t in c, -a_(k+1) for t not in c, k = |c|."""
    a = weights(n) if a is None else a
    c = np.arange(1 << n, dtype=np.int64)
    k = np.zeros(1 << n, dtype=np.int64)
    for t in range(n):
        k += (c >> t) & 1
    inside = ((c[None, :] >> np.arange(n, dtype=np.int64)[:, None]) & 1) == 1
    return np.where(inside, a[k][None, :], -a[k + 1][None, :]).reshape(n, 1 << n)


def shapley_from_values(values, n):
    """values [..., >= 2^n] (entry c: the value of the coalition whose present players are c's set bits) -> phi [..., n],
    float64, in the centred form phi_t = sum_c coef_t(c) (v(c) - v(2^n - 1))."""
    v = np.asarray(values, dtype=np.float64)[..., :1 << n]
    d = v - v[..., (1 << n) - 1:(1 << n)]
    return d @ coefficients(n).T


def shapley_by_permutations(values, n):
    """The definition: player t's marginal contribution, averaged over all n! orders of arrival.  values [2^n]."""
    v = np.asarray(values, dtype=np.float64)
    phi = np.zeros(n, dtype=np.float64)
    for order in itertools.permutations(range(n)):
        c = 0
        for t in order:
            phi[t] += v[c | (1 << t)] - v[c]
            c |= 1 << t
    return phi / math.factorial(n)


def chunks_of(n):
    return 1 << (n - CHUNK_LOG) if n > CHUNK_LOG else 1


def phi_bound(values, n):
    """The module docstring's bound -> (bound [..., n], M [..., n])."""
    v = np.asarray(values, dtype=np.float64)[..., :1 << n]
    d = np.abs(v - v[..., (1 << n) - 1:(1 << n)])
    M = d @ np.abs(coefficients(n)).T
    return (2 * U32 + (72 + chunks_of(n) + (1 << n)) * U64) * M + 2.0 ** -149, M


# ------------------------------------------------------------------------------------------------- masks from coalitions
def players_of(start_u, start_i, play_u, play_i, S_u, S_i, P):
    """-> (start_u, start_i within S, [(side, slot)] in player order): the set bits of play below S and not in start,
    the user side's ascending first, then the item side's, the lowest-numbered P of them.  Python ints."""
    su, si = (start_u & M64) & ((1 << S_u) - 1), (start_i & M64) & ((1 << S_i) - 1)
    pu = (play_u & M64) & ((1 << S_u) - 1) & ~su
    pi = (play_i & M64) & ((1 << S_i) - 1) & ~si
    players = [(0, s) for s in range(S_u) if (pu >> s) & 1] + [(1, s) for s in range(S_i) if (pi >> s) & 1]
    return su, si, players[:P]


def coalition_masks(start_u, start_i, play_u, play_i, S_u, S_i, P):
    """-> (n, n_u, mask_u int64 [2^n], mask_i int64 [2^n]): coalition c's masks are start | (the players whose bit in c
    is clear), by numpy bit operations."""
    su, si, players = players_of(start_u, start_i, play_u, play_i, S_u, S_i, P)
    n = len(players)
    c = np.arange(1 << n, dtype=np.uint64)
    masks = [np.full(1 << n, su, dtype=np.uint64), np.full(1 << n, si, dtype=np.uint64)]
    for t, (side, slot) in enumerate(players):
        absent = ((c >> np.uint64(t)) & np.uint64(1)) ^ np.uint64(1)
        masks[side] |= absent << np.uint64(slot)
    return n, sum(1 for side, _ in players if side == 0), masks[0].view(np.int64), masks[1].view(np.int64)


# ------------------------------------------------------------------------------------------------------ a float64 scorer
def _pooled64(s, idx, masks):
    z = np.concatenate([s['z'][idx].double().numpy(), s['z_pad'].double().numpy().reshape(1, -1)])
    lg = np.concatenate([s['logit'][idx].double().numpy(), [float(s['logit_pad'])]])
    sel = select(masks, z.shape[0] - 1, int(s['R']))                                # [V, R]
    l = lg[sel]
    e = np.exp(l - l.max(-1, keepdims=True))
    a = e / e.sum(-1, keepdims=True)
    o = np.einsum('vr,vrl->vl', a, z[sel])
    return o if s.get('own') is None else o + s['own'][idx].double().numpy()[None, :]


def values64(d, u, i, mask_u, mask_i, chunk=4096):
    """The float64 score of pair (u, i) under every (mask_u[v], mask_i[v]) -> float64 [V]."""
    W1, b1, w = (d[k].double().numpy() for k in ('W1', 'b1', 'w'))
    out = []
    for c0 in range(0, len(mask_u), chunk):
        x = _pooled64(d['user'], u, mask_u[c0:c0 + chunk]) * _pooled64(d['item'], i, mask_i[c0:c0 + chunk])
        out.append(np.maximum(x @ W1.T + b1, 0.0) @ w)
    sc = np.concatenate(out)
    sc = sc + (float(d['q_bias'][u]) if d['q_bias'] is not None else 0.0)
    return sc + (float(d['c_bias'][i]) if d['c_bias'] is not None else 0.0)


# ===================================================================================================== cases and inputs
# name -> dict(shape=(R_u, S_u, R_i, S_i, L), n_p, P, own, biases, seed, players=[(n_u, n_i) per pair number],
# start=None | 'pulls' (slots already removed that pull slide-ins in / put pad slots into the list), layout: how the
# players' slots are picked).  The twelve pairs come first (narre_whatif_ref.whatif_inputs); a pair's masks go with the
# PAIR, not with its place in the call.  Between them: n = 0, 1, 2, 4, 5, 10, 16; 9, 10, 11, 12 around the 1,024-coalition
# chunk; L at both edges of every fragment class; R = 1, 3, 10; S = R, R + n and 64 with R = 2; one-side games of either
# side and two-side games of (1, 1), (3, 2), (10, 6), (0, 5); start empty and not; own and biases NULL and not; lists
# with pad slots (S = R, and start leaving fewer than R).
_one = lambda ns: [(k, 0) for k in ns]
CASES = {
    'user-n0-10-L32': dict(shape=(10, 20, 10, 10, 32), n_p=12, P=10, players=_one([0, 1, 2, 4, 5, 10, 9, 3, 7, 8, 6, 10])),
    'item-R3-S3-L17': dict(shape=(3, 3, 3, 3, 17), n_p=12, P=3, own=False, biases=False,
                           players=[(0, k % 4) for k in range(12)]),
    'two-1-1-R1-L8': dict(shape=(1, 2, 1, 2, 8), n_p=12, P=2, players=[(1, 1)] * 12),
    'two-3-2-start-L33': dict(shape=(10, 12, 10, 12, 33), n_p=12, P=5, start='pulls', players=[(3, 2)] * 12, seed=1),
    'two-10-6-L16': dict(shape=(10, 20, 10, 16, 16), n_p=3, P=16, players=[(10, 6)] * 12),
    'two-0-5-L48': dict(shape=(10, 10, 10, 10, 48), n_p=12, P=5, biases=False, players=[(0, 5)] * 12),
    'user-S64-R2-L49': dict(shape=(2, 64, 10, 10, 49), n_p=12, P=5, own=False, players=_one([5] * 12), layout='far'),
    'user-67-pairs-L64': dict(shape=(10, 12, 10, 12, 64), n_p=67, P=10, players=_one([10, 5, 2, 0, 7, 1, 10, 4, 9, 3, 8, 6])),
    'user-chunk-edge-L16': dict(shape=(10, 22, 10, 10, 16), n_p=4, P=12, start='pulls', players=_one([9, 10, 11, 12] * 3)),
    'item-n7-pads-L1': dict(shape=(10, 10, 10, 10, 1), n_p=5, P=10, start='pulls', players=[(0, 7)] * 12),
}


def build_case(name):
    """A case's inputs -> dict: whatif_inputs' sides, head and pair walk, per pair start_u / start_i / play_u / play_i
    (int64 [n_p]), P, 'n' (the players each pair plays), and the float64 reference of its twelve distinct pairs:
    values64 [12][2^n], phi64, bound.  Asserts what keeps the GPU comparison from being vacuous: in float64 at least
    half of the case's players have |phi| above 1,000 times their own bound, and no pair with a player has all its
    values equal."""
    spec = CASES[name]
    R_u, S_u, R_i, S_i, L = spec['shape']
    d = whatif_inputs(R_u, S_u, R_i, S_i, L, 1, spec['n_p'], spec.get('seed', 0), biases=spec.get('biases', True),
                      own=spec.get('own', True))
    d.pop('drop_u'), d.pop('drop_i')
    P = spec['P']
    start_u, start_i, play_u, play_i = [], [], [], []
    for k in range(N_U * N_I):
        n_u, n_i = spec['players'][k]
        su = si = 0
        if spec.get('start') == 'pulls':                      # slot 0 and the last attended slot of either side are gone
            su, si = 1 | (1 << (R_u - 1)), 1 | (1 << (R_i - 1))
        free_u = [s for s in range(S_u) if not (su >> s) & 1]
        free_i = [s for s in range(S_i) if not (si >> s) & 1]
        if spec.get('layout') == 'far':                       # R = 2, S = 64: slots 0 .. 3 and one that is never reached
            picks_u = free_u[:n_u - 1] + [40]
        else:
            picks_u = free_u[k % 2:k % 2 + n_u] if len(free_u) >= n_u + k % 2 else free_u[:n_u]
        picks_i = free_i[:n_i]
        assert len(picks_u) == n_u and len(picks_i) == n_i, (name, k)
        pu, pi = sum(1 << s for s in picks_u), sum(1 << s for s in picks_i)
        # bits that must be ignored ride along: one >= S (where S < 64) and, with a start, start's own
        if S_u < 64:
            pu |= 1 << S_u
        if S_i < 64:
            pi |= 1 << 63
        pu, pi = pu | (su if n_u else 0), pi | (si if n_i else 0)
        start_u.append(as_i64(su)), start_i.append(as_i64(si)), play_u.append(as_i64(pu)), play_i.append(as_i64(pi))
    pair = (d['u_idx'] * N_I + d['i_idx'])
    pick = lambda vals: torch.tensor(vals, dtype=torch.int64)[pair].contiguous()
    d.update(start_u=pick(start_u), start_i=pick(start_i), play_u=pick(play_u), play_i=pick(play_i), P=P,
             shape=(S_u, R_u, S_i, R_i), name=name)
    # (whatif_inputs' head and logits need no scaling for the condition below: it holds at every case as drawn)
    # the float64 reference of the distinct pairs the call holds
    ref, strong, players = {}, 0, 0
    for k in sorted(set(pair.tolist())):
        n, n_u, mu, mi = coalition_masks(start_u[k], start_i[k], play_u[k], play_i[k], S_u, S_i, P)
        assert (n_u, n - n_u) == tuple(spec['players'][k]), (name, k, n, n_u)
        v = values64(d, k // N_I, k % N_I, mu, mi)
        phi = shapley_from_values(v, n)
        bound, _ = phi_bound(v, n)
        assert n == 0 or v.max() > v.min(), (name, k)
        strong, players = strong + int((np.abs(phi) > 1000 * bound).sum()), players + n
        ref[k] = dict(n=n, n_u=n_u, mask_u=mu, mask_i=mi, values=v, phi=phi, bound=bound)
    assert 2 * strong >= players > 0, (name, strong, players)
    d.update(ref=ref, pair=pair, n=torch.tensor([ref[k]['n'] for k in pair.tolist()], dtype=torch.int32),
             strong=(strong, players))
    return d
