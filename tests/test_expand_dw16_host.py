"""CPU: K25h (csrc/expand_dw16.hip) before it runs on a GPU -- the host-side shape query and refusals of the C entry
on host buffers (a refusal precedes any launch, nothing is read), fold_batchnorm(fuse_expand_depthwise=True) on all four
backbones (what it arms, the unchanged state_dict, no stale reference, beside the other 16-bit options), the loaders'
signatures, and the armed copy on the CPU, where every layer refuses."""
import ctypes
import inspect

import pytest
import torch

from metrabs_amd import _lib
from test_backbone_option_combos_host import H16_OPTS, NAMES, _net, fold, signature, stale_references, subsets

OK, E_NULL, E_SHAPE, E_DTYPE, E_PARAM, E_ALIGN = 0, -1, -2, -3, -4, -6
F32, F16, BF16 = 0, 1, 2

_store = (ctypes.c_char * (1 << 18))()
_base = (ctypes.addressof(_store) + 255) & ~255
# 16-byte aligned and far enough apart that no tensor of the shapes below overlaps another
X, Y, W1, B1, WD, B2, MEAN = (_base + i * 32768 for i in range(7))

OPTS = H16_OPTS + ('fuse_expand_depthwise',)   # the 16-bit family with the new option
# the armed pairs, from the architecture tables: the stride-1 MBConv blocks with an expand (EFFNETV2: 5 + 9 + 14 of -S,
# 9 + 19 + 24 + 7 of -L), MobileNetV3's stride-1 3x3 blocks with an expand (72 at 64x64; 200, 184, 184, 480, 672 at 16x16)
PAIRS = {'efficientnetv2-s': 28, 'efficientnetv2-l': 59, 'mobilenetv3': 6, 'resnet18': 0}


def _call(lib, x=X, dtype=F16, w1=W1, b1=B1, act1=0, wd=WD, b2=B2, act2=0, B=1, Cin=8, Cmid=8, H=4, W=4, y=Y,
          mean=None, mapping=None):
    args = (x, dtype, w1, b1, act1, wd, b2, act2, B, Cin, Cmid, H, W, y, mean, None)
    return lib.mtr_expand_dw16(*args) if mapping is None else lib.mtr_expand_dw16_opts(*args, mapping)


def test_the_shape_query_accepts_exactly_the_domain():
    from metrabs_amd import kernels
    lib = _lib.load()
    q = lib.mtr_expand_dw16_lds_bytes
    for H, W in [(16, 16), (8, 8), (4, 4), (8, 16), (16, 4)]:
        assert 0 < q(1, 8, 8, H, W) <= 160 * 1024, (H, W)
        assert kernels.k11_takes_block_kernel(H, W)
    for H, W in [(32, 32), (12, 12), (24, 24), (6, 8)]:
        assert q(1, 8, 8, H, W) == 0, (H, W)
    assert kernels.k11_takes_block_kernel(32, 32)   # K11's block kernel takes it; K25h stops at 256 positions
    assert q(1, 12, 8, 8, 8) == 0 and q(1, 8, 0, 8, 8) == 0 and q(1, 0, 8, 8, 8) == 0
    assert q(0, 8, 8, 8, 8) == 0 and q(-1, 8, 8, 8, 8) == 0
    assert q(1 << 21, 8, 8, 8, 8) == 0 and q((1 << 21) - 1, 8, 8, 8, 8) > 0   # B Cmid < 2^24: K11's own limit
    # every power-of-two block plane of at most 256 positions, and nothing else up to 64 x 64
    for H in range(4, 65, 4):
        for W in range(4, 65, 4):
            want = kernels.k11_takes_block_kernel(H, W) and H * W <= 256
            assert (q(2, 16, 24, H, W) > 0) == want, (H, W)
    # the entry agrees with the query
    for H, W in [(16, 16), (8, 16), (16, 4), (4, 4)]:
        assert _call(lib, B=0, H=H, W=W) == OK
    for H, W in [(32, 32), (12, 12), (24, 24), (6, 8)]:
        assert _call(lib, B=0, H=H, W=W) == E_SHAPE and _call(lib, B=1, H=H, W=W) == E_SHAPE
    assert _call(lib, Cin=12) == E_SHAPE and _call(lib, Cmid=0) == E_SHAPE and _call(lib, B=-1) == E_SHAPE


def test_unknown_activation_codes_are_refused_before_anything_else_runs():
    """As tests/test_act_code_refusals.py asks of every entry with an `int act` (this one spells its two codes
    act1_code and act2_code): 0 .. 3 with B = 0 are accepted, -1 and 4 are MTR_E_PARAM, on host buffers."""
    lib = _lib.load()
    for which in ('act1', 'act2'):
        assert [_call(lib, B=0, **{which: a}) for a in range(4)] == [OK] * 4
        assert _call(lib, **{which: -1}) == E_PARAM and _call(lib, **{which: 4}) == E_PARAM
        assert _call(lib, B=0, **{which: 4}) == E_PARAM   # (the argument checks come before "B == 0")
    assert [_call(lib, B=0, mapping=m) for m in (-1, 0, 1)] == [OK] * 3
    assert _call(lib, mapping=2) == E_PARAM and _call(lib, mapping=-2) == E_PARAM


def test_null_pointers_dtypes_misalignment_and_overlap_are_refused():
    lib = _lib.load()
    for name in ('x', 'w1', 'b1', 'wd', 'b2', 'y'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, B=0, mean=None) == OK and _call(lib, B=0, mean=MEAN) == OK   # the mean is optional
    assert _call(lib, dtype=F32) == E_DTYPE and _call(lib, dtype=3) == E_DTYPE
    assert _call(lib, B=0, dtype=BF16) == OK
    for name in ('x', 'w1', 'y'):
        assert _call(lib, **{name: globals()[name.upper()] + 8}) == E_ALIGN, name
    for name, base in (('b1', B1), ('wd', WD), ('b2', B2), ('mean', MEAN)):
        assert _call(lib, **{name: base + 2}) == E_ALIGN, name
    assert _call(lib, y=X) == E_PARAM and _call(lib, B=0, y=X) == E_PARAM          # y is x
    assert _call(lib, B=2, y=X + 256) == E_PARAM and _call(lib, B=2, x=X + 256, y=X) == E_PARAM   # a partial overlap
    assert _call(lib, B=0, y=X + 256) == OK                                        # (two empty ranges)
    # the order: NULL, dtype, shape, parameters, alignment, overlap
    assert _call(lib, x=None, dtype=F32) == E_NULL
    assert _call(lib, dtype=F32, H=12, W=12) == E_DTYPE
    assert _call(lib, H=12, W=12, act1=7) == E_SHAPE
    assert _call(lib, act2=7, x=X + 8) == E_PARAM
    assert _call(lib, x=X + 16, y=X) == E_PARAM and _call(lib, x=X + 8, y=X) == E_ALIGN


def test_the_option_needs_a_16bit_copy_and_is_off_by_default():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters['fuse_expand_depthwise'].default is False, fn.__name__
    net = _net('efficientnetv2-s')
    with pytest.raises(ValueError, match='fuse_expand_depthwise=True needs a 16-bit copy'):
        backbones.fold_batchnorm(net, fused_epilogue=True, fuse_expand_depthwise=True)
    with pytest.raises(ValueError):
        backbones.fold_batchnorm(net, fuse_expand_depthwise=True)
    with pytest.raises(ValueError, match='load_crop_model: fuse_expand_depthwise=True needs dtype='):
        loading.load_crop_model('/nonexistent', fuse_expand_depthwise=True)
    with pytest.raises(ValueError, match='fuse_expand_depthwise=True needs dtype='):
        loading.load_multiperson_model('/nonexistent', fuse_expand_depthwise=True)
    assert ('fuse_expand_depthwise', '16bit') in backbones._OPTION_NEEDS


def _armed_pairs(copy):
    from metrabs_amd import backbones
    return [(n, m, m.hand_to[0]) for n, m in copy.named_modules() if isinstance(m, backbones.ConvBiasAct) and m.hand_to]


@pytest.mark.parametrize('name', NAMES)
def test_the_armed_pairs_are_the_stride_1_mbconv_blocks(name):
    from metrabs_amd import backbones
    plain = fold(_net(name), torch.bfloat16, ())
    armed = fold(_net(name), torch.bfloat16, ('fuse_expand_depthwise',))
    assert not _armed_pairs(plain)
    assert not any('hand_to' in m.__dict__ for m in plain.modules() if isinstance(m, backbones.ConvBiasAct))
    assert list(armed.state_dict()) == list(plain.state_dict())
    assert [(n, type(m)) for n, m in armed.named_modules()] == [(n, type(m)) for n, m in plain.named_modules()]
    assert [n for n, _ in armed.named_buffers()] == [n for n, _ in plain.named_buffers()]
    pairs = _armed_pairs(armed)
    assert len(pairs) == PAIRS[name]
    mods = dict(armed.named_modules())
    for n, e, d in pairs:
        # the expand is layer '0' of its block, the depthwise layer '1', directly behind it
        assert n.endswith('.block.0.0') and mods[n[:-len('0.0')] + '1.0'] is d, n
        assert type(e) is backbones.ConvBiasAct and isinstance(d, backbones.DepthwiseBiasAct)
        assert not e.emit_mean and e.conv.kernel_size == (1, 1) and e.conv.out_channels == d.weight.shape[0]
        assert (d.k, d.stride, d.pad, d.pads) == (3, 1, 1, None)
    # every stride-1 3x3 depthwise layer behind a 1x1 expand is armed: the others are 5x5, stride 2 (behind a folded
    # ZeroPad2d in EfficientNetV2) or the first layer of a block without an expand
    armed_dw = {id(d) for _, _, d in pairs}
    for n, m in armed.named_modules():
        if isinstance(m, backbones.DepthwiseBiasAct) and id(m) not in armed_dw:
            assert m.k == 5 or m.stride == 2 or m.pads is not None or n.endswith('.block.0.0'), n


@pytest.mark.parametrize('name', NAMES)
def test_no_stale_reference_beside_the_other_16bit_options(name):
    """In the manner of test_backbone_option_combos_host.py: every subset of the 16-bit options that holds the new
    one.  hand_to is one of the attributes stale_references follows."""
    default = signature(fold(_net(name), torch.bfloat16, ()))
    alone = signature(fold(_net(name), torch.bfloat16, ('fuse_expand_depthwise',)))
    keys = list(fold(_net(name), torch.bfloat16, ()).state_dict())
    for s in subsets(H16_OPTS):
        opts = tuple(sorted(s)) + ('fuse_expand_depthwise',)
        copy = fold(_net(name), torch.bfloat16, opts)
        assert stale_references(copy) == [], opts
        assert list(copy.state_dict()) == keys, opts
        assert len(_armed_pairs(copy)) == PAIRS[name], opts
        # no field is armed twice: the new option changes hand_to of the expands and nothing else, whatever else is on
        sig, other = signature(copy), signature(fold(_net(name), torch.bfloat16, tuple(sorted(s))))
        for mod in sig:
            for f, v in sig[mod].items():
                if alone[mod][f] != default[mod][f]:
                    assert f == 'hand_to' and v == alone[mod][f] and other[mod][f] == default[mod][f], (opts, mod, f)
                else:
                    assert v == other[mod][f], (opts, mod, f)


@pytest.mark.parametrize('name', NAMES)
def test_the_armed_copy_on_the_cpu_is_the_default_copy(name):
    plain, armed = fold(_net(name), torch.bfloat16, ()), fold(_net(name), torch.bfloat16, OPTS)
    x = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert a.dtype == torch.bfloat16 and torch.isfinite(a.float()).all()
    assert torch.equal(a, p)
    paths = {getattr(m, 'last_path', None) for m in armed.modules()}
    assert paths <= {None, 'library', 'chain'}, paths
    only = fold(_net(name), torch.bfloat16, ('fuse_expand_depthwise',))
    with torch.inference_mode():
        assert torch.equal(only(x), p)
    assert [getattr(m, 'last_path', None) for m in only.modules()] == [getattr(m, 'last_path', None)
                                                                       for m in plain.modules()]
