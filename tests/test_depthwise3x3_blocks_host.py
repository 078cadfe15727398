"""CPU: the host side of K18 (csrc/depthwise3x3_blocks.hip): the three symbols in the header, the ctypes table and
the library; argument errors through the loaded library, in K11's order, before anything could be enqueued; the C
query, kernels.depthwise3x3_blocks_supported and kernels.k11_takes_block_kernel held together over a grid; which
layers fold_batchnorm(block_depthwise=True) arms per backbone, its argument rule, unchanged keys, and the armed copy
on CPU tensors equal to the default copy."""
import ctypes
import inspect
import os
import re

import pytest
import torch

from oracle import cases

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
SYMBOLS = ['mtr_depthwise3x3_blocks_bias_act', 'mtr_depthwise3x3_blocks_bias_act_opts',
           'mtr_depthwise3x3_blocks_supported']
E_NULL, E_SHAPE, E_DTYPE, E_PARAM, E_ALIGN = -1, -2, -3, -4, -6


def test_symbols_in_the_header_the_ctypes_table_and_the_library(hip_lib):
    from conftest import ROOT
    from metrabs_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'metrabs_hip.h')).read()
    for name in SYMBOLS:
        assert re.search(r'\bint %s\(' % name, header), name
        assert name in _lib.SIGNATURES
        assert getattr(hip_lib, name).argtypes == _lib.SIGNATURES[name][1]
    n = lambda name: len(_lib.SIGNATURES[name][1])
    assert (n(SYMBOLS[0]), n(SYMBOLS[1]), n(SYMBOLS[2])) == (12, 13, 9)
    # the header's parameter lists have as many parameters as the table
    for name in SYMBOLS:
        params = re.search(r'\bint %s\(([^;]*)\);' % name, header, flags=re.S).group(1)
        assert len(re.sub(r'/\*.*?\*/', '', params, flags=re.S).split(',')) == n(name), name


def test_argument_errors_come_in_k11s_order(hip_lib):
    """On host pointers that are never dereferenced: every one of these returns before a launch (no GPU here)."""
    f = hip_lib.mtr_depthwise3x3_blocks_bias_act_opts
    g = hip_lib.mtr_depthwise3x3_blocks_bias_act
    buf = torch.zeros(64)
    p = (buf.data_ptr() + 15) // 16 * 16
    call = lambda x=p, dtype=0, w=p, b=p, act=0, B=2, C=3, H=12, W=12, y=p, bc=0: \
        f(x, dtype, w, b, act, B, C, H, W, y, None, None, bc)
    assert call(x=None) == call(w=None) == call(b=None) == call(y=None) == E_NULL
    assert call(x=None, H=0, dtype=9, bc=3) == E_NULL                       # NULL comes first
    assert call(B=-1) == call(C=0) == call(H=0) == call(W=0) == E_SHAPE
    assert call(H=0, bc=3, dtype=9, x=p + 4) == E_SHAPE                     # then the dimensions
    assert call(bc=3) == call(bc=-1) == call(bc=16) == E_PARAM
    assert call(act=4) == call(act=-1) == E_PARAM
    assert call(bc=3, W=10, dtype=9, x=p + 4) == E_PARAM                    # then the parameters
    assert call(W=10) == call(W=6) == call(W=132) == call(H=129) == call(H=132) == E_SHAPE
    assert call(W=10, dtype=9, x=p + 4) == E_SHAPE                          # then what K18 does not take
    assert call(B=1 << 22, C=4) == E_SHAPE                                  # 2^24 planes
    assert call(bc=8) == E_PARAM and call(bc=8, dtype=1) == E_SHAPE         # 8 columns: 16 bits, W % 8 == 0
    assert call(x=p + 4) == call(y=p + 8) == call(x=p + 2, dtype=1) == E_ALIGN
    assert call(dtype=9, x=p + 4) == E_ALIGN                                # then the alignment
    assert call(B=0) == 0 and call(B=0, dtype=1, W=16, bc=8) == 0           # an empty batch: nothing to launch
    assert call(dtype=3) == call(dtype=-1) == call(dtype=3, bc=8, W=16) == E_DTYPE   # the dtype last, as in K11
    assert g(None, 0, p, p, 0, 2, 3, 12, 12, p, None, None) == E_NULL
    assert g(p, 0, p, p, 0, 2, 3, 12, 10, p, None, None) == E_SHAPE
    assert g(p + 4, 0, p, p, 0, 2, 3, 12, 12, p, None, None) == E_ALIGN
    assert g(p, 0, p, p, 0, 0, 3, 12, 12, p, None, None) == 0


def _k11_block_restated(H, W):
    """launch_depthwise's condition (csrc/depthwise.hip), written out the slow way."""
    if H % 4 or W % 4:
        return False
    pow2 = [1, 2, 4, 8, 16, 32, 64, 128, 256]
    return W // 4 in pow2 and H // 4 in pow2 and W // 4 <= 16 and (W // 4) * (H // 4) <= 64


def test_the_query_and_its_restatements_agree_over_a_grid(hip_lib):
    from metrabs_amd import _lib, kernels
    cols = ctypes.c_int(-1)
    q = lambda *a: hip_lib.mtr_depthwise3x3_blocks_supported(*a, ctypes.addressof(cols))
    assert hip_lib.mtr_depthwise3x3_blocks_supported(0, 12, 12, 1, 1, 1, 1, 1, None) == E_NULL
    pads = [(1, 1, 1, 1), (0, 0, 0, 0), (0, 1, 0, 1), (0, 2, 0, 2), (1, 0, 1, 0), (1, 1, 1, 0), (0, 1, 1, 1)]
    yes = 0
    for H in range(1, 137):
        for W in range(1, 137):
            takes = H <= 128 and W <= 128 and W % 4 == 0
            assert kernels.k11_takes_block_kernel(H, W) == _k11_block_restated(H, W)
            for stride in (1, 2):
                for pad in pads:   # (left, right, top, bottom)
                    pl, pr, pt, pb = pad
                    code = q(0, H, W, stride, pt, pl, pb, pr)
                    want = takes and stride == 1 and pad == (1, 1, 1, 1)
                    assert code == (0 if want else E_SHAPE), (H, W, stride, pad)
                    assert cols.value == (4 if want else 0)   # f32: 4 columns
                    assert kernels.depthwise3x3_blocks_supported(F32, H, W, stride, pad) == want
                    yes += want
            if kernels.k11_takes_block_kernel(H, W):   # what K11's block kernel takes, K18 would take as well
                assert takes and W <= 64
    assert yes == 128 * 32
    assert kernels.depthwise3x3_blocks_supported(F32, 12, 12, 1, 1) and kernels.depthwise3x3_blocks_supported(F16, 12, 12)
    assert not kernels.depthwise3x3_blocks_supported(F32, 12, 12, 1, 1, data_ptr=4)
    assert not kernels.depthwise3x3_blocks_supported(torch.float64, 12, 12)
    for dtype in (F32, F16, BF16):   # the block shape `auto` resolves to: 8 columns only in 16 bits where W % 8 == 0
        for W in (8, 16, 24, 28, 64, 128):
            assert q(_lib.dtype_code(dtype), 24, W, 1, 1, 1, 1, 1) == 0
            assert cols.value in (4, 8) and (cols.value == 4 or (dtype != F32 and W % 8 == 0))
            assert kernels.depthwise3x3_blocks_plan(dtype, 24, W) == cols.value
    assert kernels.depthwise3x3_blocks_plan(F32, 24, 26) is None and kernels.depthwise3x3_blocks_plan(F16, 130, 24) is None
    assert q(5, 24, 24, 1, 1, 1, 1, 1) == E_DTYPE and q(5, 24, 22, 1, 1, 1, 1, 1) == E_SHAPE
    assert q(0, 24, 24, 3, 1, 1, 1, 1) == q(0, 24, 24, 1, 2, 1, 1, 1) == q(0, 24, 24, 1, 1, 1, 3, 1) == E_PARAM
    assert q(0, 0, 24, 1, 1, 1, 1, 1) == E_SHAPE
    # the planes the issue is about
    for H, W in [(24, 24), (12, 12), (128, 128), (64, 64)]:
        assert kernels.depthwise3x3_blocks_supported(F32, H, W) and not kernels.k11_takes_block_kernel(H, W)
    for H, W in [(16, 16), (8, 8), (4, 4), (32, 32), (16, 64), (64, 4)]:
        assert kernels.k11_takes_block_kernel(H, W)


def test_wrapper_signatures():
    from metrabs_amd import backbones, kernels, loading
    sig = inspect.signature(kernels.depthwise3x3_blocks_bias_act)
    assert list(sig.parameters) == ['x', 'weight', 'bias', 'act', 'want_mean', 'block_cols']
    assert sig.parameters['want_mean'].default is False and sig.parameters['block_cols'].default is None
    assert list(inspect.signature(kernels.depthwise3x3_bias_act).parameters) == \
        ['x', 'weight', 'bias', 'act', 'stride', 'pad', 'want_mean']
    for fn in (loading.load_crop_model, loading.load_multiperson_model, backbones.fold_batchnorm):
        assert inspect.signature(fn).parameters['block_depthwise'].default is False
    with pytest.raises(RuntimeError):   # no CPU fallback
        kernels.depthwise3x3_blocks_bias_act(torch.zeros(1, 2, 12, 12), torch.zeros(2, 1, 3, 3), torch.zeros(2), None)


def _net(name):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.build_backbone(name).eval()


def _dw(net):
    from metrabs_amd import backbones
    return [m for m in net.modules() if isinstance(m, backbones.DepthwiseBiasAct)]


def test_fold_batchnorm_argument_rule():
    from metrabs_amd import backbones
    net = _net('mobilenetv3')
    with pytest.raises(ValueError, match='block_depthwise'):
        backbones.fold_batchnorm(net, block_depthwise=True)
    with pytest.raises(ValueError, match='block_depthwise'):
        backbones.fold_batchnorm(net, fused_epilogue=False, block_depthwise=True)
    for dtype in (None, F16, BF16):
        c = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, block_depthwise=True)
        assert any(m.block_depthwise for m in _dw(c))
    c = backbones.fold_batchnorm(_net('efficientnetv2-s'), fused_epilogue=True, dtype=F16, block_depthwise=True,
                                 fuse_stem=True, fuse_blocks=True)   # independent of the other options
    assert any(m.block_depthwise for m in _dw(c))


# 3x3 depthwise layers: (armed, all); the others are the stride-2 layers (with or without a folded ZeroPad2d)
ARMED = {'efficientnetv2-s': (28, 30), 'efficientnetv2-l': (59, 61), 'mobilenetv3': (7, 9), 'resnet18': (0, 0)}


@pytest.mark.parametrize('name', sorted(ARMED))
def test_which_layers_are_armed_and_the_keys_stay(name):
    from metrabs_amd import backbones
    D = backbones.DepthwiseBiasAct
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, block_depthwise=True)
    assert list(plain.state_dict()) == list(armed.state_dict())
    for (k, a), b in zip(plain.state_dict().items(), armed.state_dict().values()):
        assert torch.equal(a, b), k
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    assert [n for n, _ in plain.named_modules()] == [n for n, _ in armed.named_modules()]
    assert [n for n, _ in plain.named_buffers()] == [n for n, _ in armed.named_buffers()]
    assert not any(m.block_depthwise for m in _dw(plain))
    for m in _dw(armed):
        assert m.block_depthwise is (m.k == 3 and m.stride == 1 and m.pad == 1 and m.pads is None)
        assert m.last_path is None
    k3 = [m for m in _dw(armed) if m.k == 3]
    assert (sum(m.block_depthwise for m in k3), len(k3)) == ARMED[name]
    assert not any(m.block_depthwise for m in _dw(armed) if m.k == 5)
    assert D.use_k18 is True and isinstance(D.k18_slower, frozenset) and not D.k18_slower


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'mobilenetv3'])
def test_cpu_tensors_take_the_library_path_with_the_default_copys_bits(name):
    from metrabs_amd import backbones
    net = _net(name)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, block_depthwise=True)
    x = torch.rand(2, 3, 96, 96, generator=cases.gen(3))
    with torch.inference_mode():
        a, b = plain(x), armed(x)
    assert torch.equal(a, b)
    assert {m.last_path for m in _dw(armed)} == {'library'}
    assert [getattr(m, 'last_path', None) for m in plain.modules()] == \
        [getattr(m, 'last_path', None) for m in armed.modules()]
