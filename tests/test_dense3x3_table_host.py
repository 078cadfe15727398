"""CPU: backbones.DENSE3X3_KERNELS, the one table behind the f32 dense 3x3 kernels (K21, K19, K22), and the layer body
that reads it (Dense3x3BiasAct): every row names things that exist, its stride and Cin multiple are the C entry's own,
path() asks the armed kernels in the table's order, and fold_batchnorm builds the module trees it built before the
table existed (the counts below were recorded from the three separate classes and fold steps)."""
import collections
import inspect
import itertools

import pytest
import torch

OPTS = ('split3x3', 'winograd3x3', 'strided3x3')
# class names over modules() of the copy folded with fused_epilogue=True alone
PLAIN = {
    'efficientnetv2-s': {'Conv2d': 140, 'ConvBNAct': 110, 'ConvBiasAct': 80, 'DepthwiseBiasAct': 30,
                         'FusedMBConv': 10, 'Identity': 183, 'MBConv': 30, 'Preproc': 1, 'Sequential': 48,
                         'SiLU': 102, 'Sigmoid': 30, 'SqueezeExcite': 30},
    'resnet18': {'BasicBlock': 8, 'Conv2d': 20, 'ConvBNAct': 20, 'ConvBiasAct': 20, 'Identity': 29, 'MaxPool2d': 1,
                 'ReLU': 9, 'Sequential': 1},
    'mobilenetv3': {'Conv2d': 48, 'ConvBNAct': 47, 'ConvBiasAct': 32, 'DepthwiseBiasAct': 15, 'Hardsigmoid': 8,
                    'Hardswish': 21, 'Identity': 79, 'MBv3Block': 15, 'Preproc': 1, 'ReLU': 19, 'Sequential': 16,
                    'SqueezeExcite': 8},
}
# the ConvBiasAct layers each option replaces: (stride-1 layers with Cin % 4 == 0, all of them with Cin % 8 == 0 too;
# stride-2 layers with Cin % 4 == 0)
LAYERS = {'efficientnetv2-s': (8, 2), 'resnet18': (13, 3), 'mobilenetv3': (0, 0)}


def _expected(name, split, winograd, strided):
    """Split layers are taken before Winograd layers, so with both on every stride-1 layer is a split layer."""
    s1, s2 = LAYERS[name]
    want = dict(PLAIN[name])
    new = {'SplitConv3x3BiasAct': s1 if split else 0,
           'WinogradConv3x3BiasAct': s1 if winograd and not split else 0,
           'StridedConv3x3BiasAct': s2 if strided else 0}
    want['ConvBiasAct'] -= sum(new.values())
    want.update({k: v for k, v in new.items() if v})
    return want


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


def test_the_rows_name_what_exists_in_priority_order(hip_lib):
    from metrabs_amd import backbones, kernels
    table = backbones.DENSE3X3_KERNELS
    assert list(table) == ['k21', 'k19', 'k22']
    params = inspect.signature(backbones.fold_batchnorm).parameters
    for kernel, row in table.items():
        assert row['option'] in params and params[row['option']].default is False
        assert callable(getattr(kernels, row['pack'])) and callable(getattr(kernels, row['fn']))
        assert hasattr(hip_lib, row['query'])
        cls = getattr(backbones, row['cls'])
        assert issubclass(cls, backbones.Dense3x3BiasAct) and cls.kernel == kernel
        assert isinstance(getattr(cls, row['switch']), bool) and isinstance(getattr(cls, row['slower']), frozenset)
    assert backbones.Dense3x3BiasAct.classes() == tuple(getattr(backbones, r['cls']) for r in table.values())
    assert issubclass(backbones.SplitConv3x3BiasAct, backbones.WinogradConv3x3BiasAct)


def test_stride_and_cin_multiple_are_the_entrys_own(hip_lib):
    from metrabs_amd import backbones
    for kernel, row in backbones.DENSE3X3_KERNELS.items():
        q = getattr(hip_lib, row['query'])                       # (B, Cin, Cout, H, W)
        assert q(1, 8, 5, 8, 8) > 0, kernel
        assert q(1, 6, 5, 8, 8) == 0, kernel
        for cin in (4, 6, 8, 12, 16):
            assert (q(1, cin, 5, 8, 8) > 0) == (cin % row['cin_multiple'] == 0), (kernel, cin)
        assert (q(1, 4, 5, 8, 8) == 0) == (kernel == 'k21')
        # a row of four columns is a whole 16-byte group of a stride-1 output and half a group of a stride-2 one
        assert (q(1, 8, 5, 8, 4) > 0) == (row['stride'] == 1), kernel
        conv = lambda cin, s: torch.nn.Conv2d(cin, 5, 3, stride=s, padding=1, bias=False)
        cls = getattr(backbones, row['cls'])
        assert cls.applies_to(conv(row['cin_multiple'], row['stride']))
        assert not cls.applies_to(conv(row['cin_multiple'], 3 - row['stride']))
        assert not cls.applies_to(conv(row['cin_multiple'] + 2, row['stride']))


def _stub(layer, allowed):
    layer.takes = lambda kernel, x: kernel in allowed


def test_path_asks_the_armed_kernels_in_table_order():
    from metrabs_amd import backbones
    B = backbones
    net = _net('efficientnetv2-s')
    both = B.fold_batchnorm(net, fused_epilogue=True, split3x3=True, winograd3x3=True)
    m = next(k for k in both.modules() if isinstance(k, B.SplitConv3x3BiasAct) and k.conv.in_channels == 24)
    x = torch.zeros(1, 24, 8, 8)
    base = B.ConvBiasAct.path(m, x)
    assert base == 'library' and m.armed() == ('k21', 'k19')
    for kernel in m.armed():                                     # one slot per kernel, named by the row
        slot = B.DENSE3X3_KERNELS[kernel]['slot']
        assert getattr(m, slot, None) is None
        assert m.packed_weight(kernel) is getattr(m, slot)[1] and m.packed_weight(kernel) is getattr(m, slot)[1]
    assert m._w3s[1] is m.weight_split3() and m._wu[1] is m.weight_u() and m._w3s[1].shape != m._wu[1].shape
    assert not m.k21_takes(x) and not m.k19_takes(x) and m.path(x) == base       # on the CPU no kernel takes anything
    _stub(m, {'k21', 'k19', 'k22'})
    assert m.path(x) == 'k21'
    _stub(m, {'k19', 'k22'})
    assert m.path(x) == 'k19'
    _stub(m, {'k22'})                                                            # never a stride-1 layer's
    assert m.path(x) == base
    _stub(m, {'k21', 'k19'})
    assert m.path(x, defer_epilogue=True) == B.ConvBiasAct.path(m, x, defer_epilogue=True)
    assert m.path(x, pre=m) == B.ConvBiasAct.path(m, x, pre=m)
    out = torch.zeros(1, m.conv.out_channels, 8, 8)
    assert m.path(x, residual=out) == 'k21'
    assert m.path(x, residual=out[:, :, :4]) == B.ConvBiasAct.path(m, x, residual=out[:, :, :4])   # no skip of that shape

    alone = B.fold_batchnorm(net, fused_epilogue=True, split3x3=True)
    m = next(k for k in alone.modules() if isinstance(k, B.SplitConv3x3BiasAct) and k.conv.in_channels == 24)
    assert m.armed() == ('k21',) and m.k19_takes(x) is False
    _stub(m, {'k19', 'k22'})
    assert m.path(x) == base
    _stub(m, {'k21', 'k19'})
    assert m.path(x) == 'k21'

    wino = B.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    m = next(k for k in wino.modules() if type(k) is B.WinogradConv3x3BiasAct and k.conv.in_channels == 24)
    _stub(m, {'k21', 'k19', 'k22'})
    assert m.path(x) == 'k19'
    _stub(m, {'k21', 'k22'})
    assert m.path(x) == base

    strided = B.fold_batchnorm(net, fused_epilogue=True, strided3x3=True, split3x3=True, winograd3x3=True)
    m = next(k for k in strided.modules() if isinstance(k, B.StridedConv3x3BiasAct))
    x = torch.zeros(1, m.conv.in_channels, 8, 8)
    assert not m.k22_takes(x) and m.path(x) == 'library'
    _stub(m, {'k21', 'k19', 'k22'})
    assert m.path(x) == 'k22'
    half = torch.zeros(1, m.conv.out_channels, 4, 4)
    assert m.path(x, residual=half) == 'k22'                                     # the output's shape, from the stride
    assert m.path(x, residual=torch.zeros(1, m.conv.out_channels, 8, 8)) == 'library'
    _stub(m, {'k21', 'k19'})
    assert m.path(x) == 'library'


@pytest.mark.parametrize('name', list(PLAIN))
def test_every_combination_builds_the_recorded_tree(name):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    keys = list(plain.state_dict())
    for bits in itertools.product((False, True), repeat=3):
        copy = backbones.fold_batchnorm(net, fused_epilogue=True, **dict(zip(OPTS, bits)))
        got = collections.Counter(type(m).__name__ for m in copy.modules())
        assert dict(got) == _expected(name, *bits), bits
        assert list(copy.state_dict()) == keys, bits
        assert [n for n, _ in copy.named_modules()] == [n for n, _ in plain.named_modules()], bits
        for m in copy.modules():
            if isinstance(m, backbones.SplitConv3x3BiasAct):
                assert m.winograd is bits[1]
