"""CPU: the host side of K13h's deep-K configuration (csrc/conv1x1_16.hip): the two new symbols in the header, the
ctypes table and the library; mtr_conv1x1_plan16 for the deep project classes and for forced configurations; argument
errors of mtr_conv1x1_bias_act16_opts through the loaded library before anything could be enqueued; which layers
fold_batchnorm(deep_projects=True) arms per backbone, its argument rule, unchanged keys, and the armed copy on CPU
tensors equal to the default copy."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from oracle import cases

F16, BF16 = torch.float16, torch.bfloat16
E_NULL, E_SHAPE, E_DTYPE, E_PARAM, E_ALIGN = -1, -2, -3, -4, -6
# the workgroup tile of 'deepk' as built (csrc/conv1x1_16.hip: kDk16BM, kDk16BN), two waves along the channels
BM, BN = 64, 64

# (Cin, Cout, H * W, batch): the deep projects of EfficientNetV2-L at 384 px, batch 32, and of EfficientNetV2-S at
# 256 px, batch 64
CLASSES = [(768, 192, 576, 32), (1152, 224, 576, 32), (1344, 224, 576, 32), (1344, 384, 144, 32),
           (2304, 384, 144, 32), (2304, 640, 144, 32), (3840, 640, 144, 32), (960, 256, 64, 64), (1536, 256, 64, 64)]


def test_symbols_in_the_header_the_ctypes_table_and_the_library(hip_lib):
    from conftest import ROOT
    from metrabs_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'metrabs_hip.h')).read()
    want = {'mtr_conv1x1_bias_act16_opts': 14, 'mtr_conv1x1_plan16': 6}
    for name, n in want.items():
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == n
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
        params = re.search(r'\bint %s\(([^;]*)\);' % name, header, flags=re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', params, flags=re.S).split(',')) == n, name
    # the old entry keeps its prototype: the new one is that plus `int config`
    old, new = _lib.SIGNATURES['mtr_conv1x1_bias_act16'][1], _lib.SIGNATURES['mtr_conv1x1_bias_act16_opts'][1]
    assert len(old) == 13 and new[:13] == old and new[13] is ctypes.c_int
    assert _lib.SIGNATURES['mtr_conv1x1_plan16'] == _lib.SIGNATURES['mtr_conv1x1_plan']


def test_plan16(hip_lib):
    from metrabs_amd import kernels
    assert kernels.CONV1X1_16_CONFIGS == {'auto': -1, 'tall': 0, 'square': 1, 'deepk': 2}
    plan = kernels.conv1x1_16_plan
    for K, M, HW, B in CLASSES:
        assert plan(M, K, HW, B, 'deepk') == ('deepk', BM // 32, BM, BN)
        assert plan(M, K, HW, B, 'square') == ('square', 2, 128, 128)
        assert plan(M, K, HW, B, 'tall') == ('tall', 4, 128, 32)      # past 160 channels: rows of 128
        # the library's own choice is what it was: tall4 at M = 256, else 128 x 128
        assert plan(M, K, HW, B) == plan(M, K, HW, B, 'auto') == \
            (('tall', 4, 128, 32) if M == 256 else ('square', 2, 128, 128))
    for M in (8, 32, 33, 96, 160):
        w = (M + 31) // 32
        assert plan(M, 64, 64, 1) == plan(M, 64, 64, 1, 'tall') == ('tall', w, 32 * w, 32)
        assert plan(M, 64, 64, 1, 'deepk') == ('deepk', BM // 32, BM, BN)
    assert plan(256, 256, 64, 1) == ('square', 2, 128, 128)           # K < 512
    assert plan(161, 2304, 64, 1) == ('square', 2, 128, 128)
    assert plan(8, 8, 8, 0, 'deepk')[0] == 'deepk'                    # host only: an empty batch resolves too
    out = (ctypes.c_int * 4)(7, 7, 7, 7)
    f = hip_lib.mtr_conv1x1_plan16
    assert f(384, 2304, 144, 32, 2, None) == E_NULL
    assert f(384, 2304, 144, 32, 3, ctypes.addressof(out)) == E_PARAM
    assert f(384, 2304, 144, 32, -2, ctypes.addressof(out)) == E_PARAM
    assert f(0, 2304, 144, 32, 2, ctypes.addressof(out)) == E_SHAPE
    assert f(384, 0, 144, 32, 2, ctypes.addressof(out)) == f(384, 8, 0, 32, 2, ctypes.addressof(out)) == E_SHAPE
    assert f(384, 8, 8, -1, 2, ctypes.addressof(out)) == E_SHAPE
    assert list(out) == [7, 7, 7, 7]                                  # a refusal writes nothing
    with pytest.raises(KeyError):
        plan(8, 8, 8, 1, 'wide')


def test_opts_argument_errors_come_in_the_old_entrys_order(hip_lib):
    """On host pointers that are never dereferenced: every one of these returns before a launch (no GPU here)."""
    f = hip_lib.mtr_conv1x1_bias_act16_opts
    g = hip_lib.mtr_conv1x1_bias_act16
    buf = torch.zeros(64)
    p = (buf.data_ptr() + 15) // 16 * 16
    q = p + 64
    call = lambda x=p, dtype=1, w=p, b=p, gate=None, res=None, act=0, B=1, M=8, K=8, HW=16, y=q, cfg=2: \
        f(x, dtype, w, b, gate, res, act, B, M, K, HW, y, None, cfg)
    assert call(x=None) == call(w=None) == call(b=None) == call(y=None) == E_NULL
    assert call(x=None, dtype=0, cfg=9) == E_NULL                               # NULL comes first
    assert call(dtype=0) == call(dtype=3) == call(dtype=0, M=0, cfg=9) == E_DTYPE
    assert call(B=-1) == call(M=0) == call(K=0) == call(HW=0) == call(HW=36) == call(HW=49) == call(K=12) == E_SHAPE
    assert call(HW=36, cfg=9, act=7, x=p + 8) == E_SHAPE
    assert call(act=7) == call(act=-1) == E_PARAM
    for cfg in (-2, 3, 4, 100):
        assert call(cfg=cfg) == E_PARAM
        assert call(cfg=cfg, x=p + 8) == E_PARAM                                # the parameters before the alignment
    assert call(x=p + 8) == call(w=p + 8) == call(y=q + 8) == call(res=q + 8) == E_ALIGN
    assert call(b=p + 2) == call(gate=p + 2) == E_ALIGN
    assert call(y=p) == call(res=p) == E_PARAM                                  # y or the residual aliases x
    for cfg in (-1, 0, 1, 2):
        assert call(B=0, cfg=cfg) == 0                                          # an empty batch: nothing to launch
    # the old entry answers what config = -1 answers
    for kw in (dict(x=None), dict(dtype=0), dict(HW=36), dict(act=7), dict(x=p + 8), dict(y=p), dict(B=0)):
        a = dict(x=p, dtype=1, w=p, b=p, gate=None, res=None, act=0, B=1, M=8, K=8, HW=16, y=q)
        a.update(kw)
        assert g(a['x'], a['dtype'], a['w'], a['b'], a['gate'], a['res'], a['act'], a['B'], a['M'], a['K'], a['HW'],
                 a['y'], None) == call(cfg=-1, **kw)


def test_wrapper_signatures():
    from metrabs_amd import backbones, kernels, loading
    sig = inspect.signature(kernels.conv1x1_bias_act16)
    assert list(sig.parameters) == ['x', 'w', 'bias', 'act', 'gate', 'residual', 'out', 'config']
    assert sig.parameters['config'].default == 'auto'
    assert list(inspect.signature(kernels.conv1x1_16_plan).parameters) == ['M', 'K', 'HW', 'B', 'config']
    for fn in (loading.load_crop_model, loading.load_multiperson_model, backbones.fold_batchnorm):
        assert inspect.signature(fn).parameters['deep_projects'].default is False
    C = backbones.ConvBiasAct
    assert C.deep_config == 'deepk' and C.deep_projects is False and isinstance(C.k13h_deep_slower, frozenset)
    with pytest.raises(RuntimeError):   # no CPU fallback
        kernels.conv1x1_bias_act16(torch.zeros(1, 8, 4, 4, dtype=F16), torch.zeros(8, 8, dtype=F16), torch.zeros(8),
                                   None, config='deepk')


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


def _cba(net):
    from metrabs_amd import backbones
    return [m for m in net.modules() if isinstance(m, backbones.ConvBiasAct)]


def test_argument_rules(tmp_path):
    from metrabs_amd import backbones, loading
    net = _net('mobilenetv3')
    with pytest.raises(ValueError, match='deep_projects'):
        backbones.fold_batchnorm(net, deep_projects=True)
    with pytest.raises(ValueError, match='deep_projects'):
        backbones.fold_batchnorm(net, fused_epilogue=True, deep_projects=True)
    with pytest.raises(ValueError, match='deep_projects'):
        loading.load_crop_model(str(tmp_path), deep_projects=True)
    with pytest.raises(ValueError, match='deep_projects'):
        loading.load_crop_model(str(tmp_path), dtype=torch.float32, deep_projects=True)
    with pytest.raises(ValueError, match='deep_projects'):
        loading.load_multiperson_model(str(tmp_path), deep_projects=True)
    c = backbones.fold_batchnorm(_net('efficientnetv2-s'), fused_epilogue=True, dtype=F16, deep_projects=True,
                                 fuse_stem=True, fuse_blocks=True, block_depthwise=True)   # independent of the others
    assert sum(m.deep_projects for m in _cba(c)) == 15


# armed layers as (Cin, Cout): count
ARMED = {'efficientnetv2-s': {(960, 256): 1, (1536, 256): 14},
         'efficientnetv2-l': {(768, 192): 9, (1152, 224): 1, (1344, 224): 18, (1344, 384): 1, (2304, 384): 24,
                              (2304, 640): 1, (3840, 640): 6},
         'mobilenetv3': {}, 'resnet18': {}}


@pytest.mark.parametrize('dtype', [F16, BF16])
@pytest.mark.parametrize('name', sorted(ARMED))
def test_which_layers_are_armed_and_the_keys_stay(name, dtype):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, deep_projects=True)
    assert list(plain.state_dict()) == list(armed.state_dict())
    for (k, a), b in zip(plain.state_dict().items(), armed.state_dict().values()):
        assert torch.equal(a, b), k
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in armed.named_modules()]
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in armed.named_buffers()]
    # the default copy carries no armed attribute: the class default alone answers
    assert not any('deep_projects' in vars(m) for m in plain.modules())
    assert not any(m.deep_projects for m in _cba(plain))
    counts = {}
    for m in _cba(armed):
        c = m.conv
        want = (c.kernel_size == (1, 1) and c.stride == (1, 1) and c.groups == 1 and m.act is None
                and c.in_channels >= 768 and c.out_channels > 160)
        assert m.deep_projects is want and m.last_path is None
        if want:
            counts[(c.in_channels, c.out_channels)] = counts.get((c.in_channels, c.out_channels), 0) + 1
    assert counts == ARMED[name]
    assert sum(counts.values()) == {'efficientnetv2-s': 15, 'efficientnetv2-l': 60}.get(name, 0)
    assert not any('deep_projects' in vars(m) for m in armed.modules() if not isinstance(m, backbones.ConvBiasAct))


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_cpu_tensors_take_the_library_path_with_the_default_copys_bits(name):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=BF16)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=BF16, deep_projects=True)
    x = torch.rand(2, 3, 64, 64, generator=cases.gen(3))
    with torch.inference_mode():
        a, b = plain(x), armed(x)
    assert a.dtype == BF16 and torch.isfinite(a.float()).all()
    assert torch.equal(a, b)
    assert {m.last_path for m in _cba(armed)} == {'library'}
    assert [getattr(m, 'last_path', None) for m in plain.modules()] == \
        [getattr(m, 'last_path', None) for m in armed.modules()]
