"""The fit engine's turn schedule (conv variant 9, lemo_fit_step) on the host-emulated library: one step from a fresh state gives the
losses of lemo_fit_forward (which keeps layer 9 + fit_losses) to fp32 rounding and the gradients of lemo_fit_forward +
lemo_fit_backward (which runs the turn launch without losses) bit for bit; eager and graph steps and the LEMO_ENC_TURN=0 schedule walk the same trajectory to fp32 rounding."""
import pytest
import torch

import turn_common as T


@pytest.fixture(scope='module')
def prob_markers():
    import __graft_entry__ as ge
    prob = ge.small_problem(B=12)
    _, markers = ge.oracle_for(prob)
    return prob, markers


@pytest.mark.timeout(1800)
def test_step_equals_forward_backward(emu_lib, prob_markers, monkeypatch):
    prob, markers = prob_markers
    T.step_vs_forward_backward(prob, markers, 'cpu', emu_lib, monkeypatch)


@pytest.mark.timeout(1800)
def test_turn_and_chain_schedules_agree(emu_lib, prob_markers, monkeypatch):
    prob, markers = prob_markers
    new, old = (T.make_fitter(prob, markers, 'cpu', emu_lib, t, monkeypatch) for t in (True, False))
    for f in (new, old):
        f.step(3, use_graph=False)
    Ln, Lo = new.losses(), old.losses()
    for k in Lo:
        assert abs(Ln[k] - Lo[k]) <= 1e-5 * max(abs(Lo[k]), 1e-30), (k, Ln[k], Lo[k])
    d = (new.params75() - old.params75()).abs().max()
    assert float(d) <= 1e-5, float(d)
