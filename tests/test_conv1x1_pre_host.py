"""CPU: K13's input prologue as far as it needs no GPU: the plans of the project shapes that
inherit the prologue, which FusedMBConv blocks backbones.fold_batchnorm arms on an f32 copy, that arming changes neither
the module tree nor the state dict, and that an armed copy on CPU tensors runs the chain with the unarmed bits."""
import pytest
import torch
from torch import nn

from metrabs_amd import backbones, kernels
from metrabs_amd.backbones import FusedMBConv


def test_plans_of_the_project_classes():
    """The four FusedMBConv project classes of EfficientNetV2-S at batch 64 (M, K, HW): the whole of M in one workgroup,
    so the prologue is computed once per element."""
    for M, K, HW in [(48, 96, 4096), (48, 192, 4096), (64, 192, 1024), (64, 256, 1024)]:
        name, waves, bm, bn = kernels.conv1x1_plan(M, K, HW, 64)
        # (the two classes on 64x64 maps measured faster streamed, the two on 32x32 maps did not: DESIGN.md section 18)
        assert name == ('stream' if HW == 4096 else 'tall') and bm >= M and waves == (M + 31) // 32
    assert kernels.CONV1X1_CONFIGS['tall'] == 2 and kernels.CONV1X1_CONFIGS['stream'] == 4
    # the streaming configuration takes all four (a weight of 18 - 64 KB); two column passes per workgroup at 64x64
    for M, K, HW, bn in [(48, 96, 4096, 256), (48, 192, 4096, 256), (64, 192, 1024, 128), (64, 256, 1024, 128)]:
        assert kernels.conv1x1_plan(M, K, HW, 64, 'stream') == ('stream', (M + 31) // 32, (M + 31) // 32 * 32, bn)
    # ... and says so where the weight does not fit its 64 KB of LDS, or M is past three tiles
    assert kernels.conv1x1_plan(72, 192, 32, 3, 'stream') == kernels.conv1x1_plan(72, 192, 32, 3, 'tall')
    assert kernels.conv1x1_plan(64, 260, 64, 3, 'stream')[0] == 'tall'
    assert kernels.conv1x1_plan(160, 12, 16, 3, 'stream')[0] == 'tall'
    # every name resolves for every shape; a forced plan is the named one or says what it became
    for config in kernels.CONV1X1_CONFIGS:
        got = kernels.conv1x1_plan(48, 192, 4096, 64, config)[0]
        assert got in kernels.CONV1X1_CONFIGS and (config == 'auto' or got in (config, 'tall'))


def _armed(net):
    return [m for m in net.modules() if isinstance(m, FusedMBConv) and m.pre_pair]


@pytest.mark.parametrize('name,n_armed', [('efficientnetv2-s', 8), ('efficientnetv2-l', 14), ('mobilenetv3', 0),
                                          ('resnet18', 0)])
def test_which_blocks_fold_batchnorm_arms(name, n_armed):
    net = backbones.build_backbone(name).eval()
    f32 = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = _armed(f32)
    assert len(armed) == n_armed
    for m in armed:
        first, project = m.pre_pair
        assert first is m.block[0][0] and project is m.block[1][0] and list(m.block._modules) == ['0', '1']
        assert type(first) is backbones.ConvBiasAct and first.conv.kernel_size == (3, 3) and first.act_name == 'silu'
        assert project.conv.kernel_size == (1, 1) and project.act is None
        assert not first.emit_mean and not project.emit_mean
    if n_armed:
        # stages 2 and 3 whole, stride-2 first blocks included; stage 1 (a single 3x3 per block) not
        fm = [m for m in f32.modules() if isinstance(m, FusedMBConv)]
        assert [bool(m.pre_pair) for m in fm] == [len(m.block) == 2 for m in fm]
        assert sum(m.pre_pair[0].conv.stride == (2, 2) for m in armed) == 2
    # not without the fused epilogue, not in a 16-bit copy
    assert not _armed(backbones.fold_batchnorm(net))
    assert not _armed(backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.bfloat16))
    # nothing is registered twice, no key is added
    sd = f32.state_dict()
    assert len(sd) == len(list(f32.named_parameters())) + len(list(f32.named_buffers()))
    assert not any('pre_pair' in k for k in sd)
    assert all('pre_pair' not in m._modules for m in f32.modules())


def test_armed_copy_keeps_the_tree_and_runs_the_chain_on_cpu():
    torch.manual_seed(0)
    net = nn.Sequential(FusedMBConv(8, 8, 1, 1), FusedMBConv(8, 16, 4, 2), FusedMBConv(16, 16, 4, 1),
                        FusedMBConv(16, 24, 4, 2, bottomright=True))
    for m in net.modules():
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
    net.eval()
    copy = backbones.fold_batchnorm(net, fused_epilogue=True)
    # the block behind a ZeroPad2d keeps its three modules and stays as it is
    assert [bool(m.pre_pair) for m in copy] == [False, True, True, False]
    assert list(copy.state_dict()) == [
        k for k in backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.bfloat16).state_dict()
        if not k.endswith('weight_packed')]
    x = torch.rand(2, 8, 16, 16)
    with torch.no_grad():
        armed_out = copy(x)
    assert [m.last_path for m in copy] == [None, 'chain', 'chain', None]
    assert [m.block[0][0].last_path for m in copy[1:3]] == ['library'] * 2
    try:
        FusedMBConv.use_k13_pre = False
        with torch.no_grad():
            off_out = copy(x)
    finally:
        FusedMBConv.use_k13_pre = True
    for m in copy:
        m.pre_pair = ()   # (an instance attribute over the armed one: the block as it was before)
    with torch.no_grad():
        plain_out = copy(x)
    assert torch.equal(armed_out, off_out) and torch.equal(armed_out, plain_out)
    with torch.no_grad():
        want = net(x)
    assert float((armed_out - want).abs().max()) <= 1e-4 * float(want.abs().max())
    assert FusedMBConv.k13_pre_slower == frozenset() or all(len(k) == 6 for k in FusedMBConv.k13_pre_slower)
