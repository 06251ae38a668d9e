"""Every hand-written 3x3 convolution kernel on the MI355X across image shapes, against float64 (tests/conv_shapes_common.py: elementwise
error bound, NaN sentinels on borders / guards / scratch, two-launch determinism, refusals).

The encoder image of the fit and PROX engines is H = 3 n81 + 2, W = B + 15 (fitting.py, prox.py); B varies (PROX tail windows are
shorter than batch_size, long clips pass the split kernels' W <= 136), and each kernel tiles the image its own way.  The widths below
are W = B + 15 for B in {10, 17, 50, 100, 113, 119, 120, 121}; each kernel adds the edges of its own tiling."""
import pytest
import torch

import conv_shapes_common as C

pytestmark = pytest.mark.gpu

H0 = 245                                       # 3 * 81 + 2
B_WIDTHS = [(10, 25), (17, 32), (50, 65), (100, 115), (113, 128), (119, 134), (120, 135), (121, 136)]
MAIN = [(H0, W, f'B{b}') for b, W in B_WIDTHS]
SMALL = [(7, 41, 'small odd H'), (2, 65, 'H = 2')]

SPLIT_SHAPES = MAIN + SMALL + [
    (1, 129, 'P = 129: one block + 1 px'), (1, 128, 'H = 1, P = 128 exactly'), (2, 64, 'P = 128 exactly (W = 64)'),
    (H0, 137, 'refusal: W = 137 (B = 122)'), (H0, 150, 'refusal: W = 150'), (7, 17, 'refusal: P = 119 < 128')]
FP32_SHAPES = [s for s in MAIN if s[1] in (25, 115, 136)] + SMALL + [(H0, 150, 'W = 150: past the split limit, the LDS-tiled refuses')]
PAIR_SHAPES = [(H0, 25, 'B10'), (H0, 115, 'B100'), (H0, 136, 'B121'), (240, 126, 'H = 0 mod 10, W = 0 mod 14'),
               (241, 127, 'H = 1 mod 10, W = 1 mod 14'), (239, 125, 'H = 9 mod 10, W = 13 mod 14'), (H0, 150, 'W = 150 (wide clip)'),
               (11, 15, 'one tile + 1 row / column'), (2, 65, 'H = 2')]
WINO_SHAPES = [(H0, 25, 'B10, H odd W odd'), (H0, 136, 'B121, H odd W even'), (244, 135, 'H even W odd'), (244, 136, 'H even W even'),
               (H0, 150, 'W = 150'), (2, 25, 'H = 2'), (3, 26, 'H = 3, W even'), (5, 1, 'W = 1'), (1, 64, 'refusal: H = 1')]
C1_SHAPES = [(H0, 25), (H0, 136), (H0, 150), (7, 41), (2, 65)]
WGRAD_SHAPES = [(H0, 135, 2, 'bs H = 490 > 256 (trainer shape)'), (H0, 25, 1, 'bs = 1, H > 256 / 1 image'),
                (100, 136, 2, 'bs H = 200 < 256'), (128, 65, 2, 'bs H = 256 exactly'), (7, 41, 3, 'bs H = 21')]


def _ids(shapes):
    return [f'{s[0]}x{s[1]}-{s[2].split(":")[0].replace(" ", "")}' for s in shapes]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs the MI355X'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def lib(dev):
    from lemo_amd import _hip
    lib = _hip.get_lib()
    assert not lib.is_emu
    yield lib
    print('\nworst elementwise error / mag and max err / max ref per arithmetic:',
          {k: (f'{a:.2e}', f'{r:.2e}') for k, (a, r) in sorted(C.Rec.worst.items())})


@pytest.mark.parametrize('kernel', ['split_bf16', 'split_f16'])
@pytest.mark.parametrize('H,W,why', SPLIT_SHAPES, ids=_ids(SPLIT_SHAPES))
def test_split_kernels(lib, dev, kernel, H, W, why):
    for cin, cout in C.SINGLE[kernel][1]:
        for epi in C.SINGLE[kernel][2]:
            C.run_single(lib, dev, kernel, H, W, cin, cout, epi, refuse=why.startswith('refusal'))


@pytest.mark.parametrize('kernel', ['mfma_v0', 'mfma_v1', 'mfma_lds'])
@pytest.mark.parametrize('H,W,why', FP32_SHAPES, ids=_ids(FP32_SHAPES))
def test_fp32_kernels(lib, dev, kernel, H, W, why):
    for cin, cout in C.SINGLE[kernel][1]:
        for epi in C.SINGLE[kernel][2]:
            C.run_single(lib, dev, kernel, H, W, cin, cout, epi, refuse=kernel == 'mfma_lds' and 'LDS-tiled refuses' in why)


@pytest.mark.parametrize('ks', [2, 9, 72])            # 72 = 9 taps x 8 channel groups: one slice per (tap, group) of a 64-channel input
@pytest.mark.parametrize('H,W,why', [(H0, 115, 'B100'), (7, 41, 'small odd H')], ids=['245x115', '7x41'])
def test_splitk(lib, dev, ks, H, W, why):
    for cin, cout in C.SINGLE['splitk'][1]:
        for epi in (0, 1, 2):
            C.run_single(lib, dev, 'splitk', H, W, cin, cout, epi, ks=ks)


@pytest.mark.parametrize('H,W,why', PAIR_SHAPES, ids=_ids(PAIR_SHAPES))
def test_pair(lib, dev, H, W, why):
    for epi in (0, 1):
        C.run_pair(lib, dev, H, W, epi)


@pytest.mark.parametrize('H,W,why', WINO_SHAPES, ids=_ids(WINO_SHAPES))
def test_wino(lib, dev, H, W, why):
    for epi in (0, 1):
        C.run_single(lib, dev, 'wino_f16', H, W, 64, 64, epi, refuse=why.startswith('refusal'))


@pytest.mark.parametrize('H,W', C1_SHAPES)
def test_c1_and_tail3(lib, dev, H, W):
    C.run_c1(lib, dev, H, W)
    C.run_enc_tail3(lib, dev, H, W)


@pytest.mark.parametrize('H,W,bs,why', WGRAD_SHAPES, ids=[f'{s[0]}x{s[1]}_bs{s[2]}' for s in WGRAD_SHAPES])
def test_wgrad(lib, dev, H, W, bs, why):
    for ca, cb in [(32, 32), (64, 32), (32, 64), (64, 64), (32, 1), (1, 1)]:
        for bias_b in (0, 1):
            C.run_wgrad(lib, dev, H, W, bs, ca, cb, bias_b)


def test_wgrad_refusals(lib, dev):
    C.wgrad_refuses(lib, dev, 4, 158, 64, 64)           # W > 157 for the MFMA form
    C.wgrad_refuses(lib, dev, 4, 4, 64, 1)


# the infilling AE on one 210 x 135 clip image (bench.py's ae_finetune shape): levels 210 x 135 -> 105 x 68 -> 53 x 34 -> 27 x 17 -> 14 x 9
AE_LEVELS = [(210, 135, 32, 32, None, 'level 0, H even W odd'), (105, 68, 32, 64, (210, 135), 'level 1, H odd W even'),
             (53, 34, 64, 128, (105, 68), 'level 2, odd / even'), (27, 17, 128, 256, None, 'level 3, odd / odd'),
             (14, 9, 256, 256, (27, 17), 'level 4, even / odd')]
AE_GEOS = [(0, 0, 0), (1, 2, 8), (2, 1, 8), (3, 2, 4)]          # the engine's own choice; 32 x 32 / 32 x 64 / 16 x 16 tiles with K slices


@pytest.mark.parametrize('f16', [False, True], ids=['fp32', 'f16'])
@pytest.mark.parametrize('geo', AE_GEOS, ids=[f'mt{g[0]}pt{g[1]}ks{g[2]}' for g in AE_GEOS])
@pytest.mark.parametrize('H,W,cin,cout,fine,why', AE_LEVELS, ids=[f'{s[0]}x{s[1]}' for s in AE_LEVELS])
def test_ae_conv(lib, dev, f16, geo, H, W, cin, cout, fine, why):
    C.run_ae_conv(lib, dev, f16, H, W, cin, cout, geo, fine=fine)


@pytest.fixture(scope='module')
def amass_model():
    from lemo_amd import synthetic
    return synthetic.make_synthetic_smplx(seed=0)


@pytest.mark.parametrize('variant', [5, 9, 10])
@pytest.mark.parametrize('W', [25, 115, 136, 137, 150])
def test_engine_encoder_chain(lib, dev, amass_model, W, variant):
    """the fit engine's encoder (csrc/enc_chain.hpp) at H = 245 (81 markers), W = B + 15: 5 = pairs + split-f16 layers, 9 = + fused head and
    tail, 10 = Winograd 64 -> 64 layers; W = 137 / 150: the split kernels refuse and the unpaired layers fall back"""
    import numpy as np
    from lemo_amd import synthetic
    from lemo_amd.assets import load_assets
    from lemo_amd.vposer import make_vposer_weights
    A = load_assets()
    B = W - 15
    seq = synthetic.make_synthetic_sequence(0, B=B)
    rec = (np.random.default_rng(B).standard_normal((B, 67, 3)) * 0.3).astype(np.float32)
    prob = dict(model=amass_model, vposer_w=make_vposer_weights(2), enc_w=A['enc_w'], ids=A['ids'], Xmean=A['Xmean'], Xstd=A['Xstd'],
                seq=seq, markers_rec=rec, B=B)
    C.run_engine_encoder(lib, dev, prob, variant)
