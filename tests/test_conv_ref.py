"""The float64 conv reference and the exact pool / weight-gradient checkers of tests/conv_ref.py, on the CPU: what they
accept (fp32 ATen at small shapes) and what they must refuse (fabricated argmax and pooled-value errors)."""
import math

import pytest
import torch
import torch.nn.functional as F

from conv_ref import check_pool, check_wgrad, conv64, first_identical_window, fp32_coef


def _case(N, T, E, V, seed, zero_pad=True):
    g = torch.Generator().manual_seed(seed)
    table = (torch.rand((V, E), generator=g) - 0.5) * 0.2
    if zero_pad:
        table[0] = 0.0
    w = (torch.rand((100, 1, 3, E), generator=g) - 0.5) * (2 * math.sqrt(6.0 / (3 * E + 300 * E)))
    b = (torch.rand(100, generator=g) - 0.5) * 0.1
    idx = torch.randint(0, V, (N, T), generator=g)
    idx[0, T // 2:] = 0
    return idx, table, w, b


def _aten(idx, table, w, b):
    """fp32 ATen: pooled and the first-max argmax, -1 where pooled == 0 (the kernels' convention)."""
    y = F.conv2d(F.embedding(idx, table).unsqueeze(1), w, b, padding=(2, 0)).squeeze(-1)     # [N, F, P]
    pooled, arg = F.max_pool1d(F.relu(y), y.size(2), return_indices=True)
    pooled, arg = pooled.squeeze(-1), arg.squeeze(-1)
    return pooled, torch.where(pooled > 0, arg, torch.full_like(arg, -1)), y


def test_conv64_matches_float64_conv2d():
    idx, table, w, b = _case(3, 9, 12, 20, 1)
    y, S = conv64(idx, table, w, b)
    ref = F.conv2d(F.embedding(idx, table.double()).unsqueeze(1), w.double(), b.double(), padding=(2, 0)).squeeze(-1)
    assert y.shape == ref.shape == (3, 100, 11)
    torch.testing.assert_close(y, ref, rtol=1e-13, atol=1e-15)
    sref = F.conv2d(F.embedding(idx, table.double().abs()).unsqueeze(1), w.double().abs(), b.double().abs(),
                    padding=(2, 0)).squeeze(-1)
    torch.testing.assert_close(S, sref, rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('N,T,E,V', [(3, 1, 4, 7), (2, 40, 6, 30), (3, 37, 20, 50), (2, 129, 64, 90)])
def test_fp32_aten_passes(N, T, E, V):
    idx, table, w, b = _case(N, T, E, V, N * 100 + T)
    pooled, arg, _ = _aten(idx, table, w, b)
    assert check_pool(idx, table, w, b, pooled, arg) <= 1.0


def test_first_identical_window_counts_outside_taps_as_zero_rows():
    table = torch.tensor([[0.0, 0.0], [1.0, 2.0], [3.0, 4.0]])
    idx = torch.tensor([[0, 0, 1, 0, 0, 2]])
    # positions 0..7 read (out, out, 0) (out, 0, 0) (0, 0, 1) (0, 1, 0) (1, 0, 0) (0, 0, 2) (0, 2, out) (2, out, out)
    assert first_identical_window(idx, table).tolist() == [[0, 0, 2, 3, 4, 5, 6, 7]]


def _tied():
    """All-padding tail over a zero row 0 and a bias that beats every real window: ties at every padding window."""
    idx, table, w, b = _case(2, 50, 8, 30, 5)
    table, w = table.abs(), -w.abs()                         # every real word lowers every filter
    b[:] = 1.0
    return idx, table, w, b


def test_a_later_tied_position_fails():
    idx, table, w, b = _tied()
    pooled, arg, y = _aten(idx, table, w, b)
    check_pool(idx, table, w, b, pooled, arg)
    first = first_identical_window(idx, table)
    later = first.gather(1, arg.clamp(min=0)) == arg
    # document 0 is zero-padded from word 25 on: windows 27 .. 51 are identical; ATen picks the first of them
    # wherever the bias wins; move those argmaxes to the last tied window, which holds the same value
    bad = arg.clone()
    moved = (arg[0] >= 27) & later[0]
    assert moved.any()
    bad[0, moved] = 51
    assert torch.equal(y[0, :, 51][moved], y[0].gather(1, arg[0].unsqueeze(-1)).squeeze(-1)[moved])
    with pytest.raises(AssertionError, match='first-max rule'):
        check_pool(idx, table, w, b, pooled, bad)


def test_a_neighbouring_position_fails():
    idx, table, w, b = _case(2, 40, 6, 30, 9, zero_pad=False)
    pooled, arg, _ = _aten(idx, table, w, b)
    check_pool(idx, table, w, b, pooled, arg)
    bad = torch.where(arg > 0, arg - 1, arg)
    with pytest.raises(AssertionError):
        check_pool(idx, table, w, b, pooled, bad)
    bad = torch.where((arg >= 0) & (arg < 41), arg + 1, arg)
    with pytest.raises(AssertionError):
        check_pool(idx, table, w, b, pooled, bad)


def test_a_pooled_value_off_by_ten_beta_fails():
    idx, table, w, b = _case(2, 40, 6, 30, 11)
    pooled, arg, _ = _aten(idx, table, w, b)
    y, S = conv64(idx, table, w, b)
    n, f = (arg >= 0).nonzero()[0].tolist()
    beta = fp32_coef(6) * float(S[n, f, arg[n, f]])
    bad = pooled.double().clone()
    bad[n, f] += 10 * beta
    with pytest.raises(AssertionError, match='pooled'):
        check_pool(idx, table, w, b, bad, arg)


def test_argmax_zero_where_pooled_is_zero_fails():
    idx, table, w, b = _case(2, 40, 6, 30, 13)
    b[:7] = -10.0                                            # dead filters: pooled 0, arg -1
    pooled, arg, _ = _aten(idx, table, w, b)
    assert (arg[:, :7] == -1).all()
    bad = arg.clone()
    bad[1, 3] = 0
    with pytest.raises(AssertionError, match='arg == -1 exactly where pooled == 0'):
        check_pool(idx, table, w, b, pooled, bad)


def test_wgrad64_matches_float64_autograd():
    idx, table, w, b = _case(5, 20, 8, 30, 17, zero_pad=False)
    b[:3] = -10.0
    g = torch.randn((5, 100), generator=torch.Generator().manual_seed(3))
    w64, b64 = w.double().requires_grad_(True), b.double().requires_grad_(True)
    y = F.conv2d(F.embedding(idx, table.double()).unsqueeze(1), w64, b64, padding=(2, 0)).squeeze(-1)
    pooled, arg = F.max_pool1d(F.relu(y), y.size(2), return_indices=True)
    pooled.squeeze(-1).backward(g.double())
    arg = torch.where(pooled.squeeze(-1) > 0, arg.squeeze(-1), torch.full_like(arg.squeeze(-1), -1))
    check_wgrad(idx, table, g, arg, w64.grad.float(), b64.grad.float())
    bad = w64.grad.clone()
    bad[4, 0, 1, 2] += 1e-3
    with pytest.raises(AssertionError, match='d_w'):
        check_wgrad(idx, table, g, arg, bad, b64.grad)
