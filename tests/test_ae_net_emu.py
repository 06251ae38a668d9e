"""CPU suite: the finetune engine and the batch trainer of the infilling autoencoder share one network description
(csrc/ae_engine.hpp) -- their forwards agree bit for bit on the host emulator, and the layout sizes they report are pinned."""
import pytest

import ae_net_common as N


@pytest.mark.parametrize('H,W,K', N.SHAPES)
def test_finetune_and_trainer_forwards_agree_bit_for_bit(emu_lib, H, W, K):
    N.assert_same_network(emu_lib, H, W, K)


def test_layout_sizes_are_pinned(emu_lib):
    """parameter count, training-state size and both engines' workspace sizes: the values the engines returned before they shared
    their layout code"""
    assert emu_lib.ae_n_param() == N.N_PARAM
    assert emu_lib.aetrain_state_floats() == N.STATE_FLOATS
    for (H, W), want in N.AE_WS_FLOATS.items():
        assert emu_lib.ae_ws_floats(H, W) == want, (H, W)
    for (H, W), row in N.AETRAIN_WS_FLOATS.items():
        for bs, want in zip(N.AETRAIN_BS, row):
            assert emu_lib.aetrain_ws_floats(H, W, bs) == want, (H, W, bs)
