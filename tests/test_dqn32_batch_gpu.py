"""The fp32 forward's results do not depend on the batch size: fc1 and fc2 run
k_fc32_mfma_small up to 2 048 rows and k_fc32_mfma above, and both add every
output's products in the same order, so a row's Q-values and features have the
same bits in a batch on either side of the threshold (random real weights:
integer probes would not notice an order)."""
import pytest
import torch

import learner_cases as LC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('h,w,c', [(5, 5, 8), (4, 33, 8)])
def test_rows_are_bit_equal_across_the_fc_kernels(h, w, c):
    from marlenv import DQNForward
    torch.manual_seed(h * 100 + w)
    net = DQNForward(LC.TorchDQN(h, w, c, 3).state_dict(), h, w, c, 3, precision='fp32')
    g = torch.Generator().manual_seed(7)
    obs = (torch.rand((2304, h, w, c), generator=g) < 0.25).to(torch.uint8).cuda()
    q_big, f_big = net(obs).clone(), net.forward_features(obs).clone()      # 2 304 rows: k_fc32_mfma
    assert float(q_big.abs().max()) > 0 and not torch.equal(q_big, q_big.round())
    for B in (1, 70, 512, 2047, 2048):                                       # k_fc32_mfma_small
        sub = obs[:B].contiguous()
        assert torch.equal(net(sub), q_big[:B]), B
        assert torch.equal(net.forward_features(sub), f_big[:B]), B
    assert torch.equal(net(obs[:2049].contiguous()), q_big[:2049])           # the first size above the threshold
