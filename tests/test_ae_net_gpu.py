"""GPU suite: the finetune engine and the batch trainer of the infilling autoencoder run one network -- the same parameters and
images give the same reconstruction bits from lemo_ae_forward_clip and lemo_aetrain_eval on an MI355X."""
import pytest

import ae_net_common as N
from lemo_amd import _hip

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('H,W,K', N.SHAPES)
def test_finetune_and_trainer_forwards_agree_bit_for_bit(H, W, K):
    N.assert_same_network(_hip.get_lib(), H, W, K, dev='cuda')
