"""The encoder's turn launch (csrc/conv_turn_kernels.hip) on the host-emulated build, at ragged and odd shapes: float64 bounds for z
and d(pre-act 9), d(pre-act 10) bit-identical to lemo_smooth_loss on the kernel's own z, NaN sentinels, two-launch determinism and
refusals (tests/turn_common.py)."""
import pytest
import torch

import turn_common as T

DEV = torch.device('cpu')

# (H, W, why)
SHAPES = [(12, 12, 'one whole tile'), (13, 25, 'H, W = 1 mod 12: remainder row and column'), (11, 14, 'H = 11 mod 12, W = 2 mod 12'),
          (25, 12, 'three tile rows, one column, W = 12'), (3, 2, 'W = 2: one time difference'), (1, 40, 'H = 1'),
          (9, 1, 'refusal: W = 1'), (0, 12, 'refusal: H = 0')]


@pytest.fixture(scope='module')
def lib(emu_lib):
    return emu_lib


@pytest.mark.parametrize('H,W,why', SHAPES, ids=[f'{s[0]}x{s[1]}' for s in SHAPES])
def test_turn(lib, H, W, why):
    r = T.run_turn(lib, DEV, H, W)
    assert (r is None) == why.startswith('refusal')


def test_turn_tall_narrow(lib):
    """the encoder's height (H = 3 * 81 + 2 = 245, 21 tile rows, the last one 5 rows) at the smallest clip width"""
    T.run_turn(lib, DEV, 245, 12)
