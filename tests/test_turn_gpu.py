"""The encoder's turn launch (csrc/conv_turn_kernels.hip) and the fit engine's turn schedule on the MI355X (tests/turn_common.py):
the launch at the encoder's shapes against float64, one `step` against `forward` + `backward` (losses to rounding, gradients bit for bit), and
100-step bit-identity of graph replay vs eager runs and across two engines."""
import pytest
import torch

import turn_common as T

pytestmark = pytest.mark.gpu

SHAPES = [(245, 134, 'B119: the headline'), (245, 25, 'B10'), (245, 136, 'B121'), (240, 120, 'H, W = 0 mod 12'),
          (241, 121, 'H, W = 1 mod 12'), (13, 2, 'W = 2'), (245, 1, 'refusal: W = 1')]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib():
    from lemo_amd import _hip
    return _hip.get_lib()


@pytest.mark.parametrize('H,W,why', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_turn_vs_float64(lib, dev, H, W, why):
    r = T.run_turn(lib, dev, H, W)
    assert (r is None) == why.startswith('refusal')
    if r is not None:
        print(f'turn {H} x {W}: z err ratio {r[0][0]:.3e} (rel {r[0][1]:.2e}), d(pre-act 9) {r[1][0]:.3e} (rel {r[1][1]:.2e})')


@pytest.fixture(scope='module')
def prob_markers():
    import __graft_entry__ as ge
    prob = ge.small_problem(B=119)
    _, markers = ge.oracle_for(prob)
    return prob, markers


@pytest.mark.parametrize('use_graph', [False, True])
def test_step_equals_forward_backward(lib, dev, prob_markers, monkeypatch, use_graph):
    prob, markers = prob_markers
    s = torch.cuda.Stream(dev)                   # graph capture needs a stream other than the legacy default one
    with torch.cuda.stream(s):
        wl = T.step_vs_forward_backward(prob, markers, dev, lib, monkeypatch, use_graph=use_graph)
    s.synchronize()
    print(f'step vs forward + backward: losses {wl:.2e}, gradients bit-identical')


def test_100_steps_graph_eager_two_engines_bit_identical(lib, dev, prob_markers, monkeypatch):
    prob, markers = prob_markers
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):
        a, b, c = (T.make_fitter(prob, markers, dev, lib, True, monkeypatch) for _ in range(3))
        a.step(100, use_graph=True)
        b.step(100, use_graph=False)
        c.step(100, use_graph=True)
    s.synchronize()
    assert torch.equal(a.params75(), b.params75()), 'graph replay vs eager'
    assert torch.equal(a.params75(), c.params75()), 'two engines'
    La, Lb = a.losses(), b.losses()
    assert all(La[k] == Lb[k] for k in La)
