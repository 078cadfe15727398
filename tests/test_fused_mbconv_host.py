"""CPU: the fuse_blocks option of backbones.fold_batchnorm (K16h) as far as it needs no GPU: its
argument rule, which blocks it arms, that it changes neither the module tree nor the state dict, and that an armed copy
on CPU tensors runs the two-module chain and returns the unarmed copy's bits."""
import pytest
import torch
from torch import nn

from metrabs_amd import backbones
from metrabs_amd.backbones import FusedMBConv


def _net():
    torch.manual_seed(0)
    net = nn.Sequential(FusedMBConv(8, 8, 1, 1),                      # expand ratio 1: a single 3x3, nothing to fuse
                        FusedMBConv(8, 16, 4, 2),                     # stride 2, no skip
                        FusedMBConv(16, 16, 4, 1),                    # the skip
                        FusedMBConv(16, 24, 4, 2, bottomright=True))  # behind a ZeroPad2d
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    return net.eval()


def test_fuse_blocks_needs_a_16_bit_dtype():
    net = _net()
    with pytest.raises(ValueError, match='fuse_blocks'):
        backbones.fold_batchnorm(net, fused_epilogue=True, fuse_blocks=True)
    with pytest.raises(ValueError):
        backbones.fold_batchnorm(net, fuse_blocks=True)
    backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.bfloat16, fuse_blocks=True)


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_arming_picks_the_expand_project_blocks_only(dtype):
    net = _net()
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_blocks=True)
    assert [bool(m.fused_pair) for m in armed] == [False, True, True, False]
    assert isinstance(armed[3].block[0], nn.ZeroPad2d) and list(armed[0].block._modules) == ['0']
    for m in plain:
        assert 'fused_pair' not in m.__dict__ and m.fused_pair == () and m.last_path is None
    for m in (armed[1], armed[2]):
        expand, project = m.fused_pair
        assert isinstance(m.fused_pair, tuple)
        assert expand is m.block[0][0] and isinstance(expand, backbones.Conv3x3BiasAct)
        assert project is m.block[1][0] and isinstance(project, backbones.ConvBiasAct) and project.act is None
    # the same tree, the same keys, the same tensors: nothing is registered twice, no weight is copied
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    assert sum(p.numel() for p in plain.parameters()) == sum(p.numel() for p in armed.parameters())
    assert len(list(armed.buffers())) == len(list(plain.buffers()))
    for k, v in plain.state_dict().items():
        assert torch.equal(v, armed.state_dict()[k]), k


def test_an_armed_copy_on_cpu_tensors_takes_the_chain():
    net = _net()
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.bfloat16)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.bfloat16, fuse_blocks=True)
    x = torch.rand(2, 8, 16, 16)
    with torch.no_grad():
        a, b = plain(x), armed(x)
    assert a.dtype == torch.bfloat16 and torch.equal(a, b)
    assert [m.last_path for m in armed] == [None, 'chain', 'chain', None]
    assert [m.last_path for m in plain] == [None] * 4
    assert not any(m.k16h_takes(x.bfloat16()) for m in armed)


def test_the_loaders_take_the_option(tmp_path):
    import inspect
    from metrabs_amd import loading
    for fn in (loading.load_crop_model, loading.load_multiperson_model, backbones.fold_batchnorm):
        assert inspect.signature(fn).parameters['fuse_blocks'].default is False
    with pytest.raises(ValueError, match='fuse_blocks'):
        loading.load_crop_model(str(tmp_path), fuse_blocks=True)   # refused before anything is read
