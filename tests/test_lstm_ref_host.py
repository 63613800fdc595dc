"""tests/lstm_ref.py against torch's own float64 ``nn.LSTM`` on the CPU: the reference of tests/test_gpu_lstm.py is
held to 1e-12 (hidden states, and the gate gradients against autograd), its layout helpers to being bijections, and
each of its rounding options to moving the result by more than nothing and by less than 2e-2."""
import pytest
import torch

import lstm_ref
from lstm_ref import rel

H, T = 6, 7


def _lstm(directions, seed):
    """A float64 nn.LSTM whose input IS the gate input: input size directions*4H, W_ih of direction d the identity on
    columns d*4H .. -- so that autograd's gradient with respect to the input is the gradient with respect to
    gates_in."""
    torch.manual_seed(seed)
    m = torch.nn.LSTM(directions*4*H, H, batch_first=True, bidirectional=directions == 2).double()
    with torch.no_grad():
        for d, sfx in enumerate(('', '_reverse')[:directions]):
            w = getattr(m, 'weight_ih_l0' + sfx)
            w.zero_()
            w[:, d*4*H:(d + 1)*4*H] = torch.eye(4*H, dtype=torch.float64)
            getattr(m, 'weight_hh_l0' + sfx).normal_(0, 0.5)
            getattr(m, 'bias_ih_l0' + sfx).normal_(0, 0.3)
            getattr(m, 'bias_hh_l0' + sfx).normal_(0, 0.3)
    return m


def _params(m, directions):
    sfx = ('', '_reverse')[:directions]
    w_hh = torch.stack([getattr(m, 'weight_hh_l0' + s).detach() for s in sfx])
    bias = torch.stack([(getattr(m, 'bias_ih_l0' + s) + getattr(m, 'bias_hh_l0' + s)).detach() for s in sfx])
    return w_hh, bias


@pytest.mark.parametrize('steps', [1, 2, T])
def test_unidirectional_equals_nn_lstm(steps):
    m = _lstm(1, 1)
    N = 5
    x = torch.randn(N, steps, 4*H, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(N, steps, H, dtype=torch.float64)
    want, _ = m(x)
    (want*gy).sum().backward()
    w_hh, bias = _params(m, 1)
    y, act, cs = lstm_ref.forward(x.detach(), w_hh, bias)
    assert rel(y, want) <= 1e-12
    assert rel(lstm_ref.backward(act, cs, w_hh, gy), x.grad) <= 1e-12
    # the interleaved gate order is a relabelling: nothing else about the recurrence depends on it
    assert torch.equal(lstm_ref.deinterleave(lstm_ref.interleave(act)), act)


@pytest.mark.parametrize('steps', [1, 2, T])
def test_bidirectional_is_two_groups_the_second_reversed(steps):
    m = _lstm(2, 2)
    N = 4
    x = torch.randn(N, steps, 8*H, dtype=torch.float64, requires_grad=True)
    gy = torch.randn(N, steps, 2*H, dtype=torch.float64)
    want, _ = m(x)
    (want*gy).sum().backward()
    w_hh, bias = _params(m, 2)
    gates = torch.cat([x.detach()[..., :4*H], x.detach()[..., 4*H:]])            # (2N, steps, 4H): group-major chains
    y, act, cs = lstm_ref.forward(gates, w_hh, bias, groups=2, reverse_mask=2)
    # nn.LSTM's (N, steps, 2H) output is the layout ld = 2H, group_offset = H
    assert rel(lstm_ref.place_y(y, 2, 2*H, H).view(N, steps, 2*H), want) <= 1e-12
    idx = lstm_ref.y_index(2*N, steps, H, 2, 2*H, H)
    dy = gy.reshape(-1)[idx]                                                    # (2N, steps, H) by frame
    dg = lstm_ref.backward(act, cs, w_hh, dy, groups=2, reverse_mask=2)
    assert rel(torch.cat([dg[:N], dg[N:]], dim=-1), x.grad) <= 1e-12
    # act / cs are indexed by recurrence step: the reversed group's last step is frame 0
    h_last = act[N:, steps - 1, 3*H:]*torch.tanh(cs[N:, steps - 1])
    assert rel(h_last, want[:, 0, H:]) <= 1e-12
    # without the mask the second group is a plain forward LSTM: a different result
    y0, _, _ = lstm_ref.forward(gates, w_hh, bias, groups=2, reverse_mask=0)
    assert (rel(y0[N:], y[N:]) > 1e-3) == (steps > 1) and torch.equal(y0[:N], y[:N])


def test_three_groups_mask_0b101_are_three_independent_runs():
    torch.manual_seed(3)
    per, G = 3, 3
    gates = torch.randn(G*per, T, 4*H, dtype=torch.float64)
    w_hh = 0.5*torch.randn(G, 4*H, H, dtype=torch.float64)
    bias = 0.3*torch.randn(G, 4*H, dtype=torch.float64)
    dy = torch.randn(G*per, T, H, dtype=torch.float64)
    y, act, cs = lstm_ref.forward(gates, w_hh, bias, groups=G, reverse_mask=0b101)
    dg = lstm_ref.backward(act, cs, w_hh, dy, groups=G, reverse_mask=0b101)
    for g in range(G):
        sl = slice(g*per, (g + 1)*per)
        flip = (lambda v: v.flip(1)) if g != 1 else (lambda v: v)
        y1, a1, c1 = lstm_ref.forward(flip(gates[sl]), w_hh[g:g + 1], bias[g:g + 1])
        assert torch.equal(flip(y1), y[sl]) and torch.equal(a1, act[sl]) and torch.equal(c1, cs[sl])
        assert torch.equal(flip(lstm_ref.backward(a1, c1, w_hh[g:g + 1], flip(dy[sl]))), dg[sl])
    # bias None is bias zero
    y2, _, _ = lstm_ref.forward(gates, w_hh, None, groups=G)
    y3, _, _ = lstm_ref.forward(gates, w_hh, torch.zeros_like(bias), groups=G)
    assert torch.equal(y2, y3)


def test_interleave_is_a_bijection():
    n = 4*H
    x = torch.arange(3*n, dtype=torch.float64).view(3, n)
    inter = lstm_ref.interleave(x)
    assert torch.equal(inter.sort(dim=-1).values, x) and not torch.equal(inter, x)
    assert torch.equal(lstm_ref.deinterleave(inter), x)
    assert torch.equal(lstm_ref.interleave(lstm_ref.deinterleave(x)), x)
    for u in range(H):
        for g in range(4):
            assert inter[0, 4*u + g] == x[0, g*H + u]


@pytest.mark.parametrize('groups,ld,goff', [(1, H, 0), (3, H, 4*T*H), (3, 3*H, H), (2, 2*H, H)])
def test_y_index_places_every_element_once(groups, ld, goff):
    B = 4*groups
    idx = lstm_ref.y_index(B, T, H, groups, ld, goff)
    flat = idx.reshape(-1)
    assert flat.unique().numel() == flat.numel() == B*T*H and int(flat.min()) == 0 and int(flat.max()) == B*T*H - 1
    per = B//groups
    assert int(idx[per + 2, 3, 1]) == 1*goff + (2*T + 3)*ld + 1 if groups > 1 else True
    y = torch.randn(B, T, H, dtype=torch.float64)
    assert torch.equal(lstm_ref.place_y(y, groups, ld, goff)[idx], y)


def test_each_rounding_option_moves_the_result_a_little():
    torch.manual_seed(4)
    Hh, N, S = 128, 6, 9
    # bf16-representable gate inputs, as the caller of io16 provides them
    gates = lstm_ref.round_bf16(torch.randn(2*N, S, 4*Hh)).double()
    w_hh = torch.randn(2, 4*Hh, Hh, dtype=torch.float64)/Hh**0.5
    bias = 0.1*torch.randn(2, 4*Hh, dtype=torch.float64)
    dy = torch.randn(2*N, S, Hh, dtype=torch.float64)
    kw = dict(groups=2, reverse_mask=2)
    y, act, cs = lstm_ref.forward(gates, w_hh, bias, **kw)
    dg = lstm_ref.backward(act, cs, w_hh, dy, **kw)
    yr, actr, csr = lstm_ref.forward(gates, w_hh, bias, round_operands=True, **kw)
    for a, b in ((yr, y), (actr, act), (csr, cs)):
        assert 0 < rel(a, b) < 2e-2, rel(a, b)
    assert 0 < rel(lstm_ref.backward(act, cs, w_hh, dy, round_operands=True, **kw), dg) < 2e-2
    # io16 alone: the recurrence is untouched, the saved activations are rounded
    y16, act16, cs16 = lstm_ref.forward(gates, w_hh, bias, io16=True, **kw)
    assert torch.equal(y16, y) and torch.equal(cs16, cs) and torch.equal(act16, lstm_ref.round_bf16(act))
    assert 0 < rel(act16, act) < 2e-2
    dg16, dg16r = lstm_ref.backward(act, cs, w_hh, dy, io16=True, **kw)
    assert torch.equal(dg16r, lstm_ref.round_bf16(dg16))
    assert 0 < rel(dg16, dg) < 2e-2 and 0 < rel(dg16r, dg) < 2e-2
    # both: rounding the adjoint's operand is the same rounding as storing it
    both, _ = lstm_ref.backward(act, cs, w_hh, dy, round_operands=True, io16=True, **kw)
    assert torch.equal(both, lstm_ref.backward(act, cs, w_hh, dy, round_operands=True, **kw))
    # the float32 restatement with the kernels' forms of sigmoid / tanh: float32 rounding only
    y32, act32, cs32 = lstm_ref.forward(gates, w_hh, bias, dtype=torch.float32, fast=True, **kw)
    assert y32.dtype == torch.float32
    for a, b in ((y32, y), (act32, act), (cs32, cs)):
        assert 0 < rel(a, b) < 1e-5, rel(a, b)
