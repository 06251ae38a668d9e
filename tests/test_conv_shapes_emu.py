"""The conv shape sweep (tests/conv_shapes_common.py) on the host-emulated build: the same case bodies as
tests/test_gpu_conv_shapes.py -- float64 elementwise bounds, NaN sentinels on borders / guards / scratch, two-launch determinism,
refusals -- at small shapes that hit the same tiling edges."""
import pytest
import torch

import conv_shapes_common as C

DEV = torch.device('cpu')

# (H, W, why) -- small images that reach each kernel's edges
SPLIT_SHAPES = [(2, 65, 'P = 130: one block + a 2-px tail'), (1, 128, 'H = 1, P = 128: exactly one block, no tail'),
                (3, 135, 'W = 135'), (2, 136, 'W = 136, the split limit'), (7, 41, 'odd H, 2 blocks + 31-px tail'),
                (1, 137, 'refusal: W = 137'), (7, 17, 'refusal: P = 119 < 128')]
FP32_SHAPES = [(7, 41, 'odd H'), (2, 65, 'H = 2'), (3, 136, 'W = 136')]
PAIR_SHAPES = [(10, 14, 'one whole tile'), (11, 15, 'H, W = 1 mod 10, 14'), (9, 13, 'H = 9 mod 10, W = 13 mod 14'), (3, 28, 'two tile columns, one short row')]
WINO_SHAPES = [(2, 25, 'H = 2, W odd'), (3, 26, 'H odd, W even'), (4, 7, 'H even, W odd'), (5, 1, 'W = 1: half a tile'), (1, 20, 'refusal: H = 1')]
WGRAD_SHAPES = [(7, 9, 2, 'bs H = 14 < 256'), (130, 5, 2, 'bs H = 260 > 256'), (5, 21, 1, 'bs = 1')]


def _ids(shapes):
    return [f'{s[0]}x{s[1]}' for s in shapes]


@pytest.fixture(scope='module')
def lib(emu_lib):
    return emu_lib


@pytest.mark.parametrize('kernel', ['split_bf16', 'split_f16'])
@pytest.mark.parametrize('H,W,why', SPLIT_SHAPES, ids=_ids(SPLIT_SHAPES))
def test_split_kernels(lib, kernel, H, W, why):
    for cin, cout in C.SINGLE[kernel][1]:
        for epi in C.SINGLE[kernel][2]:
            C.run_single(lib, DEV, kernel, H, W, cin, cout, epi, refuse=why.startswith('refusal'))


@pytest.mark.parametrize('kernel', ['mfma_v0', 'mfma_v1', 'mfma_lds', 'splitk'])
@pytest.mark.parametrize('H,W,why', FP32_SHAPES, ids=_ids(FP32_SHAPES))
def test_fp32_kernels(lib, kernel, H, W, why):
    for cin, cout in C.SINGLE[kernel][1]:
        for epi in C.SINGLE[kernel][2]:
            C.run_single(lib, DEV, kernel, H, W, cin, cout, epi, ks=5, refuse=kernel == 'mfma_lds' and W > 139)


@pytest.mark.parametrize('H,W,why', PAIR_SHAPES, ids=_ids(PAIR_SHAPES))
def test_pair(lib, H, W, why):
    for epi in (0, 1):
        C.run_pair(lib, DEV, H, W, epi)


@pytest.mark.parametrize('H,W,why', WINO_SHAPES, ids=_ids(WINO_SHAPES))
def test_wino(lib, H, W, why):
    for epi in (0, 1):
        C.run_single(lib, DEV, 'wino_f16', H, W, 64, 64, epi, refuse=why.startswith('refusal'))


@pytest.mark.parametrize('H,W', [(7, 41), (2, 9)])
def test_c1_and_tail3(lib, H, W):
    C.run_c1(lib, DEV, H, W)
    C.run_enc_tail3(lib, DEV, H, W)


@pytest.mark.parametrize('H,W,bs,why', WGRAD_SHAPES, ids=[f'{s[0]}x{s[1]}_bs{s[2]}' for s in WGRAD_SHAPES])
def test_wgrad(lib, H, W, bs, why):
    for ca, cb in [(32, 32), (64, 32), (32, 64), (64, 64), (32, 1), (1, 1)]:
        for bias_b in (0, 1):
            C.run_wgrad(lib, DEV, H, W, bs, ca, cb, bias_b)


def test_wgrad_refusals(lib):
    C.wgrad_refuses(lib, DEV, 4, 158, 64, 64)           # W > 157 for the MFMA form
    C.wgrad_refuses(lib, DEV, 4, 4, 64, 1)


@pytest.mark.parametrize('f16', [False, True], ids=['fp32', 'f16'])
@pytest.mark.parametrize('geo', [(0, 0, 0), (1, 2, 8), (3, 2, 4)], ids=['mt0', 'mt1pt2ks8', 'mt3pt2ks4'])
def test_ae_conv(lib, f16, geo):
    C.run_ae_conv(lib, DEV, f16, 7, 9, 32, 64, geo, fine=(13, 17))        # odd level, odd fine image
    C.run_ae_conv(lib, DEV, f16, 4, 5, 64, 64, geo, fine=(8, 9))          # even level


@pytest.mark.parametrize('variant', [5, 9, 10])
def test_engine_encoder_chain(lib, variant):
    """the fit engine's encoder (csrc/enc_chain.hpp) on a small problem: 6 markers (H = 20), B = 10 (W = 25)"""
    import numpy as np
    import __graft_entry__ as ge
    prob = ge.small_problem(B=10)
    prob['markers_rec'] = (np.random.default_rng(10).standard_normal((10, len(prob['ids']['markers67']), 3)) * 0.3).astype(np.float32)
    C.run_engine_encoder(lib, DEV, prob, variant)
