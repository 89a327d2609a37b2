"""r4r_narre_shapley on the device (csrc/narre_shapley.hip; include/r4r.h, "NARRE Shapley values"), through
ops.narre_shapley.

What decides.  The VALUES: the existing kernel -- every coalition's masks are built on the host and scored by
``ops.narre_whatif``, and out_values, out_base and out_empty must equal it bit for bit, with no tolerance.  The SHARES:
narre_shapley_ref's float64 ``shapley_from_values`` applied to the kernel's OWN fp32 values, within the bound its
docstring derives per rounding from the accumulation rule the header states.  Then exact zeros, counts, efficiency, and
the things a pair's outputs must not depend on, bit for bit.  Cases, seeds and inputs are narre_shapley_ref's
(tests/test_narre_shapley_host.py shows on the CPU that no case is vacuous)."""
import numpy as np
import pytest
import torch

from head_ref import bits_equal
from narre_search_ref import as_i64
from narre_shapley_ref import CASES, build_case, phi_bound, players_of, shapley_from_values

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _t(a):
    return None if a is None else a.contiguous().to(DEV)


def _sides(d):
    side = lambda s: dict(z=_t(s['z']), logit=_t(s['logit']), z_pad=_t(s['z_pad']), own=_t(s.get('own')),
                          logit_pad=s['logit_pad'], R=s['R'])
    return side(d['user']), side(d['item'])


def shapley(d, sel=None, values=True, **over):
    """ops.narre_shapley over a case (``sel`` picks pairs, ``over`` replaces entries) -> dict of numpy arrays."""
    from reviews4rec_amd import ops
    d = dict(d, **over)
    pick = lambda a: a if a is None or sel is None else a[sel]
    su, si = _sides(d)
    got = ops.narre_shapley(su, si, _t(pick(d['u_idx'])), _t(pick(d['i_idx'])), _t(d['W1']), _t(d['b1']), _t(d['w']),
                            play_u=_t(pick(d['play_u'])), play_i=_t(pick(d['play_i'])), start_u=_t(pick(d['start_u'])),
                            start_i=_t(pick(d['start_i'])), P=d['P'], q_bias=_t(d['q_bias']), c_bias=_t(d['c_bias']),
                            values=values)
    torch.cuda.synchronize()
    n_p = int(pick(d['u_idx']).numel())
    S_u, _, S_i, _ = d['shape']
    out = dict(zip(('phi_u', 'phi_i', 'base', 'empty', 'n', 'values'), (None if g is None else g.cpu().numpy() for g in got)))
    assert out['phi_u'].shape == (n_p, S_u) and out['phi_i'].shape == (n_p, S_i) and out['phi_u'].dtype == np.float32
    assert out['base'].shape == out['empty'].shape == out['n'].shape == (n_p,) and out['n'].dtype == np.int32
    assert (out['values'] is None) == (not values) and (not values or out['values'].shape == (n_p, 1 << d['P']))
    return out


def same_bits(a, b, what=''):
    for k in ('phi_u', 'phi_i', 'base', 'empty'):
        assert bits_equal(a[k], b[k]), (what, k)
    assert np.array_equal(a['n'], b['n']), what


def whatif_values(d, k):
    """Every coalition of pair number ``k`` through the EXISTING kernel: one ``ops.narre_whatif`` call of one pair x 2^n
    variants over host-built masks -> float32 [2^n]."""
    from reviews4rec_amd import ops
    r = d['ref'][k]
    su, si = _sides(d)
    u, i = torch.tensor([k // 4]), torch.tensor([k % 4])
    mu, mi = torch.from_numpy(r['mask_u'].copy())[None, :], torch.from_numpy(r['mask_i'].copy())[None, :]
    return ops.narre_whatif(su, si, _t(u), _t(i), _t(mu), _t(mi), _t(d['W1']), _t(d['b1']), _t(d['w']), q_bias=_t(d['q_bias']),
                            c_bias=_t(d['c_bias'])).cpu().numpy()[0]


@pytest.fixture(scope='module')
def built():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = build_case(name)                    # the float64 reference: once per case, never changed
        return cache[name]
    return get


# ---------------------------------------------------------------- values, shares, zeros, counts, efficiency
@pytest.mark.parametrize('name', sorted(CASES))
def test_values_are_the_whatif_kernels_and_shares_are_within_the_bound(built, name):
    d = built(name)
    got = shapley(d)
    S_u, _, S_i, _ = d['shape']
    pairs = d['pair'].tolist()
    assert np.array_equal(got['n'], d['n'].numpy())
    want = {k: whatif_values(d, k) for k in d['ref']}
    worst = eff = 0.0
    for p, k in enumerate(pairs):
        r = d['ref'][k]
        n = r['n']
        vals = got['values'][p, :1 << n]
        assert bits_equal(vals, want[k]), (name, p, k)                             # no tolerance
        assert bits_equal(got['base'][p:p + 1], vals[-1:]) and bits_equal(got['empty'][p:p + 1], vals[:1])
        _, _, players = players_of(int(d['start_u'][p]), int(d['start_i'][p]), int(d['play_u'][p]), int(d['play_i'][p]),
                                   S_u, S_i, d['P'])
        phi = np.array([got['phi_u' if side == 0 else 'phi_i'][p, s] for side, s in players], dtype=np.float64)
        ref = shapley_from_values(vals, n)                                          # of the kernel's OWN values
        bound, _ = phi_bound(vals, n)
        assert np.isfinite(phi).all() and (np.abs(phi - ref) <= bound).all(), (name, p, k, phi, ref, bound)
        if n:
            worst = max(worst, float((np.abs(phi - ref) / bound).max()))
            gap = abs(phi.sum() - (float(got['base'][p]) - float(got['empty'][p])))
            room = bound.sum() + 2.0 ** -53 * np.abs(phi).sum() * n
            assert gap <= room, (name, p, gap, room)
            eff = max(eff, gap / room)
        # a slot that is no player holds +0.0f exactly
        for side, key, S in ((0, 'phi_u', S_u), (1, 'phi_i', S_i)):
            free = np.array([s for s in range(S) if (side, s) not in players], dtype=np.int64)
            assert (got[key][p, free].view(np.uint32) == 0).all(), (name, p, key)
    print('%s: worst |phi - float64 of the own values| / bound %.3f, worst efficiency gap / room %.3f' % (name, worst, eff))


# ---------------------------------------------------------------- what a pair's outputs do not depend on
@pytest.mark.parametrize('name', ['user-67-pairs-L64', 'user-chunk-edge-L16', 'two-3-2-start-L33'])
def test_a_pairs_bits_depend_on_its_own_inputs_only(built, name):
    d = built(name)
    full = shapley(d)
    n_p = len(d['pair'])
    cut = lambda r, sel: {k: r[k][sel] for k in ('phi_u', 'phi_i', 'base', 'empty', 'n')}
    for p in sorted({0, 1, n_p // 2, n_p - 1}):                 # a pair alone against the same pair inside the call
        same_bits(shapley(d, sel=slice(p, p + 1)), cut(full, slice(p, p + 1)), (name, p))
    perm = torch.randperm(n_p, generator=torch.Generator().manual_seed(7))
    same_bits(shapley(d, sel=perm), cut(full, perm.numpy()), 'permuted')
    same_bits(shapley(d, values=False), full, 'out_values NULL')
    for P in sorted({min(d['P'] + 1, 16), 11, 16} - {d['P']}):  # P larger than needed: through scratch from 11 on
        if P > d['P']:
            same_bits(shapley(d, P=P, values=False), full, 'P = %d' % P)
    S_u, _, S_i, _ = d['shape']
    extra = dict(d)
    if S_u < 64:                                               # one more play bit at a slot >= S
        extra['play_u'] = d['play_u'] | (1 << (S_u + 1 if S_u < 63 else 63))
    extra['play_i'] = d['play_i'] | as_i64(1 << 63) if S_i < 64 else d['play_i']
    same_bits(shapley(extra), full, 'a play bit beyond S')
    shared = dict(d, play_u=d['play_u'] | d['start_u'], play_i=d['play_i'] | d['start_i'])
    same_bits(shapley(shared), full, "start's bits among the players")


def test_null_masks_and_null_sides(built):
    d = built('user-n0-10-L32')
    full = shapley(d)
    zero = torch.zeros_like(d['start_u'])
    same_bits(shapley(d, start_u=None, start_i=None), full, 'NULL start')
    same_bits(shapley(d, play_i=None), full, 'NULL play_i: its bits were all beyond S')
    none = shapley(d, play_u=None, play_i=None)
    assert (none['n'] == 0).all() and not none['phi_u'].any() and not none['phi_i'].any()
    assert bits_equal(none['base'], full['base']) and bits_equal(none['empty'], full['base'])
    assert bits_equal(none['values'][:, 0], full['base'])
    same_bits(shapley(d, play_u=zero, play_i=zero), none, 'empty masks')


def test_a_truncated_pair_plays_its_lowest_numbered_players(built):
    for name, P in (('two-3-2-start-L33', 4), ('two-3-2-start-L33', 2), ('user-n0-10-L32', 3), ('user-chunk-edge-L16', 10)):
        d = built(name)
        S_u, _, S_i, _ = d['shape']
        cut = shapley(d, P=P)
        want_n = np.minimum(d['n'].numpy(), P)
        assert np.array_equal(cut['n'], want_n) and (want_n < d['n'].numpy()).any()
        pu, pi = [], []
        for p in range(len(d['pair'])):                        # the same pair with only those P bits set
            _, _, players = players_of(int(d['start_u'][p]), int(d['start_i'][p]), int(d['play_u'][p]),
                                       int(d['play_i'][p]), S_u, S_i, P)
            pu.append(as_i64(sum(1 << s for side, s in players if side == 0)))
            pi.append(as_i64(sum(1 << s for side, s in players if side == 1)))
        alone = shapley(d, P=P, play_u=torch.tensor(pu), play_i=torch.tensor(pi))
        same_bits(cut, alone, (name, P))
        for p in range(len(d['pair'])):
            assert bits_equal(cut['values'][p, :1 << want_n[p]], alone['values'][p, :1 << want_n[p]])
        same_bits(shapley(d, P=16, play_u=torch.tensor(pu), play_i=torch.tensor(pi), values=False), cut, 'P = 16')


# ---------------------------------------------------------------- refusals (host addresses that are never dereferenced)
PTR = 4096
OK, ERR_ARG = 0, -1


def shapley_args(**kw):
    a = dict(z_u=PTR, logit_u=PTR, own_u=PTR, z_pad_u=PTR, logit_pad_u=0.5, n_u=3, S_u=12, R_u=10, z_i=PTR, logit_i=PTR,
             own_i=PTR, z_pad_i=PTR, logit_pad_i=-0.5, n_i=4, S_i=11, R_i=10, u_idx=PTR, i_idx=PTR, start_u=PTR,
             start_i=PTR, play_u=PTR, play_i=PTR, P=10, n_p=7, q_bias=PTR, c_bias=PTR, W1=PTR, b1=PTR, w=PTR, L=32,
             out_phi_u=PTR, out_phi_i=PTR, out_base=PTR, out_empty=PTR, out_n=PTR, out_values=PTR, scratch=PTR,
             stream=None)
    assert not set(kw) - set(a)
    a.update(kw)
    return a


def _call(args):
    from reviews4rec_amd import _lib
    lib = _lib.lib()
    assert list(args) == _lib.parse_header()['r4r_narre_shapley'][2]             # the dict IS the header's argument list
    return lib.r4r_narre_shapley(*args.values()), lib.r4r_last_error() or b''


@pytest.mark.parametrize('over, word', [
    (dict(P=0), b'P='), (dict(P=17), b'P='), (dict(P=-1), b'P='),
    (dict(n_p=1 << 21, P=10), b'out_values'), (dict(n_p=1 << 15, P=16), b'out_values'), (dict(n_p=1 << 31, P=1), b'n_p='),
    (dict(n_p=-1), b'n_p='),
    (dict(S_u=0), b'S_u='), (dict(S_u=65), b'S_u='), (dict(S_i=0), b'S_i='), (dict(S_i=65), b'S_i='),
    (dict(R_u=0), b'R_u='), (dict(R_u=13), b'R_u='), (dict(R_i=0), b'R_i='), (dict(R_i=12), b'R_i='),
    (dict(L=0), b'L='), (dict(L=65), b'L='), (dict(n_u=-1), b'n_u='), (dict(n_i=-1), b'n_i='),
    (dict(z_u=None), b'z_u'), (dict(logit_u=None), b'logit_u'), (dict(z_pad_u=None), b'z_pad_u'),
    (dict(z_i=None), b'z_i'), (dict(logit_i=None), b'logit_i'), (dict(z_pad_i=None), b'z_pad_i'),
    (dict(u_idx=None), b'null'), (dict(i_idx=None), b'null'), (dict(W1=None), b'null'), (dict(b1=None), b'null'),
    (dict(w=None), b'null'), (dict(out_base=None), b'out_base'), (dict(out_empty=None), b'out_empty'),
    (dict(out_n=None), b'out_n'), (dict(out_phi_u=None), b'out_phi_u'), (dict(out_phi_i=None), b'out_phi_i'),
    (dict(scratch=None, P=11), b'scratch'), (dict(n_u=0), b'n_u='), (dict(n_i=0), b'n_i='),
])
def test_refusals_precede_the_launch_and_name_the_entry_point(over, word):
    got, msg = _call(shapley_args(**over))
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_shapley') and word in msg, (over, got, msg)


def test_nothing_to_do_is_ok_and_enqueues_nothing():
    assert _call(shapley_args(n_p=0))[0] == OK
    nul = {k: None for k, v in shapley_args().items() if v == PTR}
    assert _call(shapley_args(n_p=0, n_u=0, n_i=0, **nul))[0] == OK
    assert _call(shapley_args(n_p=0, R_u=13))[0] == ERR_ARG                        # the shape is still checked
    got, msg = _call(shapley_args(n_p=0, P=17))
    assert got == ERR_ARG and msg.startswith(b'r4r_narre_shapley')
    # without out_values the pair count alone is held to 2^31 - 1; the largest table that fits is accepted up to there
    got, msg = _call(shapley_args(n_p=1 << 21, P=10, out_values=None, z_u=None))
    assert got == ERR_ARG and b'z_u' in msg
