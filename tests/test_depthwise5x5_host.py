"""CPU: K15 (depthwise 5x5 + bias + activation, csrc/depthwise5x5.hip) from the C entry up to fold_batchnorm,
as far as it goes without a GPU: the symbol in header / ctypes table / library, the host-side argument checks
of the entry (they come before any launch), the folded module trees, and the torch fallback of the folded
MobileNetV3 on CPU tensors."""
import os
import re

import pytest
import torch
from torch import nn

from conftest import ROOT

NAME = 'mtr_depthwise5x5_bias_act_padded'
OK, E_NULL, E_SHAPE, E_DTYPE, E_PARAM, E_ALIGN = 0, -1, -2, -3, -4, -6


@pytest.fixture(scope='module')
def lib():
    from metrabs_amd import build, _lib
    build.build_library(verbose=False)  # hipcc cross-compiles gfx950 without a GPU
    return _lib.load()


def test_symbol_in_header_ctypes_table_and_library(lib):
    from metrabs_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'metrabs_hip.h')).read()
    header = re.sub(r'/\*.*?\*/', '', header, flags=re.S)
    assert re.search(rf'^\s*int\s+{NAME}\s*\(', header, flags=re.M)
    assert NAME in _lib.SIGNATURES
    assert _lib.SIGNATURES[NAME] == _lib.SIGNATURES['mtr_depthwise3x3_bias_act_padded']  # K11's contract
    assert hasattr(lib, NAME)


def _call(lib, x=1 << 20, dtype=0, w=1 << 20, b=1 << 20, act=0, B=1, C=8, H=16, W=16, stride=1,
          pads=(2, 2, 2, 2), y=1 << 20, mean=None):
    """Pointers are never dereferenced on the host: made-up, aligned addresses do for the argument checks
    (every call here fails a check, or has B == 0, before a launch).  pads = (top, left, bottom, right)."""
    return getattr(lib, NAME)(x, dtype, w, b, act, B, C, H, W, stride, *pads, y, mean, None)


def test_argument_errors_come_before_any_launch(lib):
    for missing in ('x', 'w', 'b', 'y'):
        assert _call(lib, **{missing: None}) == E_NULL, missing
    assert _call(lib, B=-1) == E_SHAPE and _call(lib, C=0) == E_SHAPE and _call(lib, H=0) == E_SHAPE
    assert _call(lib, stride=3) == E_PARAM and _call(lib, stride=0) == E_PARAM
    for pads in [(3, 2, 2, 2), (2, 3, 2, 2), (2, 2, 4, 2), (2, 2, 2, 4), (-1, 2, 2, 2), (2, 2, 2, -1)]:
        assert _call(lib, pads=pads) == E_PARAM, pads
    assert _call(lib, H=2, pads=(1, 2, 1, 2)) == E_SHAPE              # padded plane below 5 rows
    assert _call(lib, W=18) == E_SHAPE                                # OW = 18
    assert _call(lib, W=13, stride=2, pads=(2, 2, 2, 2)) == E_SHAPE   # OW = 7
    assert _call(lib, y=(1 << 20) + 4) == E_ALIGN
    # same order as mtr_depthwise3x3_bias_act_padded: NULL, shape, stride, pads, OW, alignment
    assert _call(lib, x=None, stride=3) == E_NULL
    assert _call(lib, C=0, stride=3) == E_SHAPE
    assert _call(lib, stride=3, pads=(9, 9, 9, 9)) == E_PARAM
    assert _call(lib, W=18, y=(1 << 20) + 4) == E_SHAPE
    assert _call(lib, B=0) == OK                                      # nothing to do, no launch
    assert _call(lib, B=0, dtype=7) == OK and _call(lib, B=0, act=9) == OK  # (as K11: B == 0 returns first)
    assert _call(lib, dtype=7) == E_DTYPE                             # the dtype switch precedes the launch
    assert _call(lib, H=120) == E_SHAPE                               # padded plane above 112 rows: no LDS tile
    assert _call(lib, act=9) == E_PARAM                               # no kernel for the code: nothing launched


def _folded(name, **kw):
    from metrabs_amd import backbones
    return backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True, **kw)


def _dw(net):
    from metrabs_amd import backbones
    return [m for m in net.modules() if isinstance(m, backbones.DepthwiseBiasAct)]


def test_mobilenetv3_folds_its_5x5_layers_onto_k15():
    from metrabs_amd import backbones
    net = _folded('mobilenetv3')
    dws = _dw(net)
    assert len(dws) == 15
    five = [m for m in dws if m.k == 5]
    assert [m.weight.shape[0] for m in five] == [72, 120, 120, 672, 960, 960]
    assert [m.stride for m in five] == [2, 1, 1, 2, 1, 1]
    assert all(tuple(m.weight.shape) == (m.weight.shape[0], 1, 5, 5) and m.pad == 2 and m.pads is None for m in five)
    assert all(m.k == 3 and m.weight.shape[-1] == 3 for m in dws if m not in five)
    ses = [m for m in net.modules() if isinstance(m, backbones.SqueezeExcite)]
    for m in five:
        assert m.emit_mean and sum(1 for s in ses if len(s.mean_from) == 1 and s.mean_from[0] is m) == 1
    # a 16-bit copy keeps the 5x5 layers' parameters in f32, like K11's
    half = _folded('mobilenetv3', dtype=torch.float16)
    assert all(m.weight.dtype == torch.float32 and m.bias.dtype == torch.float32 for m in _dw(half))
    assert sum(m.k == 5 for m in _dw(half)) == 6


def _tree(net):
    return [(n, type(m).__name__) for n, m in net.named_modules()]


def test_kernel_sizes_3_gives_the_tree_without_k15(monkeypatch):
    from metrabs_amd import backbones
    assert backbones.DepthwiseBiasAct.kernel_sizes == (3, 5)
    with_k15 = _folded('mobilenetv3')
    monkeypatch.setattr(backbones.DepthwiseBiasAct, 'kernel_sizes', (3,))
    net = _folded('mobilenetv3')
    assert len(_dw(net)) == 9 and all(m.k == 3 for m in _dw(net))
    five = [m for m in net.modules() if isinstance(m, backbones.ConvBiasAct) and m.conv.kernel_size == (5, 5)]
    assert [m.conv.in_channels for m in five] == [72, 120, 120, 672, 960, 960]
    assert all(isinstance(m.conv, backbones.DepthwiseConv2d) and m.emit_mean for m in five)
    # everything else is the same, module for module
    a, b = dict(_tree(with_k15)), dict(_tree(net))
    six = [n for n, m in with_k15.named_modules() if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 5]
    assert len(six) == 6 and set(b) - set(a) == {n + '.conv' for n in six} and not set(a) - set(b)
    for n, t in a.items():
        assert b[n] == ('ConvBiasAct' if n in six else t), n
    assert all(b[n + '.conv'] == 'DepthwiseConv2d' for n in six)


def test_bottomright_padding_of_a_5x5_layer_is_folded_into_pads():
    from metrabs_amd import backbones
    blk = backbones.MBConv(16, 24, 4, 2, k=5, bottomright=True).eval()
    assert tuple(blk.block.padding.padding) == (1, 3, 1, 3)
    net = nn.Sequential(blk).eval()
    folded = backbones.fold_batchnorm(net, fused_epilogue=True)
    (dw,) = _dw(folded)
    assert dw.k == 5 and dw.stride == 2 and dw.pad == 0 and dw.pads == (1, 3, 1, 3) and dw.emit_mean
    assert isinstance(folded[0].block.padding, nn.Identity)
    # TF-'SAME' (2, 2, 2, 2) in front of an unpadded 5x5 and a padding K15 does not take
    for pad, taken in [((2, 2, 2, 2), True), ((0, 3, 0, 3), True), ((3, 1, 3, 1), False), ((2, 4, 2, 4), False)]:
        blk = backbones.MBConv(16, 24, 4, 2, k=5, bottomright=True).eval()
        blk.block.padding = nn.ZeroPad2d(pad)
        folded = backbones.fold_batchnorm(nn.Sequential(blk).eval(), fused_epilogue=True)
        (dw,) = _dw(folded)
        assert (dw.pads == pad) == taken and isinstance(folded[0].block.padding, nn.Identity) == taken, pad
    # the torch fallback pads and convolves at the real kernel size
    x = torch.rand(2, 16, 16, 16, generator=torch.Generator().manual_seed(3))
    torch.manual_seed(0)
    blk = nn.Sequential(backbones.MBConv(16, 24, 4, 2, k=5, bottomright=True)).train()
    with torch.no_grad():
        for i in range(3):   # running statistics that are not the identity
            blk(torch.rand(8, 16, 16, 16, generator=torch.Generator().manual_seed(10 + i)))
    blk.eval()
    with torch.inference_mode():
        want = blk(x)
        got = backbones.fold_batchnorm(blk, fused_epilogue=True)(x)
    assert got.shape == want.shape == (2, 24, 8, 8)
    assert float((got - want).abs().max()) <= 2e-4 * float(want.abs().max())


@pytest.mark.parametrize('name', ['effnetv2-s', 'resnet18'])
def test_backbones_without_5x5_layers_fold_as_before(name, monkeypatch):
    from metrabs_amd import backbones
    net = _folded(name)
    assert not any(getattr(m, 'k', None) == 5 for m in net.modules())
    assert not any(isinstance(m, nn.Conv2d) and m.kernel_size == (5, 5) for m in net.modules())
    monkeypatch.setattr(backbones.DepthwiseBiasAct, 'kernel_sizes', (3,))
    assert _tree(_folded(name)) == _tree(net)
    for a, b in zip(_dw(_folded(name)), _dw(net)):
        assert (a.k, a.stride, a.pad, a.pads, a.emit_mean) == (b.k, b.stride, b.pad, b.pads, b.emit_mean)


def test_folded_mobilenetv3_on_cpu_is_the_same_function():
    """The torch fallback of DepthwiseBiasAct at the real kernel size: the gate of
    test_host_logic.test_fold_batchnorm_is_the_same_function (2e-4 of the largest feature)."""
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone('mobilenetv3'), 64, 'cpu', batches=2, batch_size=4)
    fused = backbones.fold_batchnorm(net, fused_epilogue=True)
    five = [m for m in _dw(fused) if m.k == 5]
    assert len(five) == 6
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1))
    with torch.inference_mode():
        a, c = net(x), fused(x)
    assert a.shape == c.shape == (2, 1280, 2, 2)
    assert float((a - c).abs().max()) <= 2e-4 * float(a.abs().max())
    assert all(m.last_path == 'library' for m in five)
