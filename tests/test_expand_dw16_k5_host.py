"""CPU: K28h (csrc/expand_dw16_k5.hip) before it runs on a GPU -- the host-side shape query against a restatement of its
rule, the refusals of the C entry on host buffers (a refusal precedes any launch, nothing is read),
fold_batchnorm(fuse_expand_depthwise5x5=True) on all four backbones (what it arms, the unchanged state_dict, the sibling
fields left alone), the loaders' refusals, the code object's resources, and the armed copy on the CPU, where every layer
runs the chain."""
import ctypes
import inspect

import pytest
import torch

from metrabs_amd import _lib
from test_backbone_option_combos_host import H16_OPTS, NAMES, _net, fold, stale_references

OK, E_NULL, E_SHAPE, E_DTYPE, E_PARAM, E_ALIGN = 0, -1, -2, -3, -4, -6
F32, F16, BF16 = 0, 1, 2

_store = (ctypes.c_char * (1 << 18))()
_base = (ctypes.addressof(_store) + 255) & ~255
# 16-byte aligned and far enough apart that no tensor of the shapes below overlaps another
X, Y, W1, B1, WD, B2 = (_base + i * 32768 for i in range(6))

NEW = 'fuse_expand_depthwise5x5'
SIBLINGS = {'fuse_expand_depthwise': 'hand_to', 'fuse_expand_depthwise_planes': 'hand_planes_to',
            'fuse_expand_depthwise_tiles': 'hand_tiles_to'}
PAIRS = {'efficientnetv2-s': 0, 'efficientnetv2-l': 0, 'mobilenetv3': 6, 'resnet18': 0}
LDS_MAX = 160 * 1024
STAGING = 2 * 256 * 40 * 2   # two X^T buffers of 256 positions x (32 + 8) k, 16-bit


def lds_rule(Cmid, H, W, stride):
    """The entry's plane and LDS rule, restated -> the bytes of LDS of a workgroup, or 0 where it refuses.  The image
    of a channel is PH rows of LW 16-bit elements (K15's PH / PW rule with the windows read in whole 8-byte groups and the
    plane's column 0 at index 4); beside the image lie the staging buffers of phase 1 or, later in their place, 28
    weights and `units` sums per channel in f32.  64 channels where Cmid > 32 and that fits 80 KiB, else 32."""
    if stride not in (1, 2) or H <= 0 or W <= 0 or (H * W) % 8 or W % 4 or H + 4 > 112 or W + 4 > 112:
        return 0
    OH, OW = (H - 1) // stride + 1, (W - 1) // stride + 1
    if OW % 4:
        return 0
    RB, NC = (4, 3) if stride == 1 else (2, 4)
    UH = -(-OH // RB)
    units = UH * (OW // 4)
    PH = max((UH * RB - 1) * stride + 5, H + 4)
    LW = (max(stride * (OW - 4) + 4 * NC, W + 6) + 3) & ~3
    lds = lambda CM: CM * PH * LW * 2 + max(STAGING, CM * (28 + units) * 4)
    if Cmid > 32 and lds(64) <= LDS_MAX // 2:
        return lds(64)
    return lds(32) if lds(32) <= LDS_MAX else 0


def _call(lib, x=X, dtype=F16, w1=W1, b1=B1, act1=0, wd=WD, b2=B2, act2=0, B=1, Cin=8, Cmid=8, H=4, W=4, stride=1, y=Y,
          mean=None):
    return lib.mtr_expand_dw16_k5(x, dtype, w1, b1, act1, wd, b2, act2, B, Cin, Cmid, H, W, stride, y, mean, None)


def test_the_shape_query_is_the_restated_rule():
    q = _lib.load().mtr_expand_dw16_k5_lds_bytes
    for Cin, Cmid in [(8, 8), (112, 672)]:
        seen = 0
        for stride in (1, 2):
            for H in range(1, 117):
                for W in range(1, 117):
                    n = q(2, Cin, Cmid, H, W, stride)
                    assert n == lds_rule(Cmid, H, W, stride), (Cmid, H, W, stride)
                    assert n <= LDS_MAX
                    seen += n > 0
        assert seen > 500
    for H, W, s in [(32, 32, 1), (16, 16, 2), (8, 8, 1), (4, 4, 1), (32, 32, 2), (16, 16, 1), (8, 8, 2), (12, 16, 1)]:
        assert q(1, 16, 8, H, W, s) > 0 and q(1, 160, 960, H, W, s) > 0, (H, W, s)
    # the 64x64 stride-2 pair of MobileNetV3 (24 -> 72) keeps the chain: its 32-channel slice does not fit
    for H, W, s in [(64, 64, 2), (64, 64, 1), (40, 40, 1), (108, 108, 1), (112, 112, 2), (6, 6, 1), (5, 4, 1), (8, 8, 3),
                    (8, 8, 0), (8, 6, 2), (8, 12, 2)]:
        assert q(1, 16, 8, H, W, s) == 0 == lds_rule(8, H, W, s), (H, W, s)
    assert q(1, 12, 8, 8, 8, 1) == 0 and q(1, 8, 0, 8, 8, 1) == 0 and q(1, 0, 8, 8, 8, 1) == 0
    assert q(0, 8, 8, 8, 8, 1) == 0 and q(-1, 8, 8, 8, 8, 1) == 0
    assert q(1 << 27, 8, 8, 8, 8, 1) == 0 and q((1 << 27) - 1, 8, 8, 8, 8, 1) > 0   # B Cmid < 2^30: K15's own limit


def test_the_entry_refuses_by_rule_before_any_launch():
    lib = _lib.load()
    assert _call(lib, B=0) == OK and _call(lib, B=0, dtype=BF16, H=16, W=16, stride=2) == OK
    for name in ('x', 'w1', 'b1', 'wd', 'b2', 'y'):
        assert _call(lib, **{name: None}) == E_NULL, name
    assert _call(lib, dtype=F32) == E_DTYPE and _call(lib, dtype=3) == E_DTYPE
    assert _call(lib, Cin=12) == E_SHAPE
    assert _call(lib, H=5, W=4) == E_SHAPE                      # H W = 20
    assert _call(lib, stride=3) == E_SHAPE and _call(lib, stride=0) == E_SHAPE
    assert _call(lib, y=Y + 8) == E_ALIGN and _call(lib, x=X + 8) == E_ALIGN and _call(lib, w1=W1 + 8) == E_ALIGN
    for name, base in (('b1', B1), ('wd', WD), ('b2', B2), ('mean', B2 + 4096)):
        assert _call(lib, **{name: base + 2}) == E_ALIGN, name
    # a plane whose 32-channel slice does not fit 160 KiB of LDS, with and without images
    for B in (0, 1):
        assert _call(lib, B=B, H=64, W=64, stride=2) == E_SHAPE and _call(lib, B=B, H=40, W=40) == E_SHAPE
    assert _call(lib, H=3, W=4) == E_SHAPE and _call(lib, H=8, W=12, stride=2) == E_SHAPE   # H W % 8; OW % 4
    assert _call(lib, H=112, W=8) == E_SHAPE and _call(lib, Cmid=0) == E_SHAPE and _call(lib, B=-1) == E_SHAPE
    for which in ('act1', 'act2'):
        assert [_call(lib, B=0, **{which: a}) for a in range(4)] == [OK] * 4
        assert _call(lib, **{which: -1}) == E_PARAM and _call(lib, B=0, **{which: 4}) == E_PARAM
    assert lib.mtr_expand_dw16_k5_opts(X, F16, W1, B1, 0, WD, B2, 0, 0, 8, 8, 4, 4, 1, Y, None, None, 2) == E_PARAM
    for mapping in (-1, 0, 1):
        assert lib.mtr_expand_dw16_k5_opts(X, F16, W1, B1, 0, WD, B2, 0, 0, 8, 8, 4, 4, 1, Y, None, None,
                                           mapping) == OK
    assert _call(lib, y=X) == E_PARAM and _call(lib, B=2, y=X + 256) == E_PARAM     # y is x; a partial overlap
    # stride 2: x [2, 8, 8, 8] is 2048 bytes, y [2, 8, 4, 4] is 512
    assert _call(lib, B=2, H=8, W=8, stride=2, y=X + 1024) == E_PARAM
    assert _call(lib, B=2, H=8, W=8, stride=2, x=X + 256, y=X) == E_PARAM
    assert _call(lib, B=0, H=8, W=8, stride=2, x=X + 256, y=X) == OK                # (two empty ranges)
    # the order: NULL, dtype, shape, parameters, alignment, overlap
    assert _call(lib, x=None, dtype=F32) == E_NULL
    assert _call(lib, dtype=F32, H=5) == E_DTYPE
    assert _call(lib, H=5, act1=7) == E_SHAPE and _call(lib, stride=3, act1=7) == E_SHAPE
    assert _call(lib, act2=7, x=X + 8) == E_PARAM
    assert _call(lib, x=X + 16, y=X) == E_PARAM and _call(lib, x=X + 8, y=X) == E_ALIGN


def test_the_option_needs_a_16bit_copy_and_is_off_by_default():
    from metrabs_amd import backbones, loading
    for fn in (backbones.fold_batchnorm, loading.load_crop_model, loading.load_multiperson_model):
        assert inspect.signature(fn).parameters[NEW].default is False, fn.__name__
    net = _net('mobilenetv3')
    with pytest.raises(ValueError, match='fuse_expand_depthwise5x5=True needs a 16-bit copy'):
        backbones.fold_batchnorm(net, fused_epilogue=True, fuse_expand_depthwise5x5=True)
    with pytest.raises(ValueError):
        backbones.fold_batchnorm(net, fuse_expand_depthwise5x5=True)
    with pytest.raises(ValueError, match='load_crop_model: fuse_expand_depthwise5x5=True needs dtype='):
        loading.load_crop_model('/nonexistent', fuse_expand_depthwise5x5=True)
    with pytest.raises(ValueError, match='fuse_expand_depthwise5x5=True needs dtype='):
        loading.load_multiperson_model('/nonexistent', fuse_expand_depthwise5x5=True)
    assert (NEW, '16bit') in backbones._OPTION_NEEDS
    assert [o for o, _ in backbones._OPTION_NEEDS].count(NEW) == 1
    D = backbones.DepthwiseBiasAct
    assert D.use_k28h is True and isinstance(D.k28h_slower, frozenset)
    assert all(len(key) == 5 and key[4] in (1, 2) for key in D.k28h_slower)
    assert backbones.ConvBiasAct.hand_k5_to == ()
    row = backbones.EXPAND_DW_KERNELS['k28h']
    assert row == dict(option=NEW, field='hand_k5_to', takes='k28h_takes', switch='use_k28h', slower='k28h_slower',
                       fn='expand_depthwise16_k5', strided=True, mean=True)
    # every row says what its call passes, and the three earlier rows pass what they passed
    assert {k: (r['strided'], r['mean']) for k, r in backbones.EXPAND_DW_KERNELS.items()} == {
        'k25h': (False, True), 'k26h': (False, True), 'k27h': (True, False), 'k28h': (True, True)}


def _armed(copy, field):
    from metrabs_amd import backbones
    return [(n, m, getattr(m, field)[0]) for n, m in copy.named_modules()
            if isinstance(m, backbones.ConvBiasAct) and getattr(m, field)]


@pytest.mark.parametrize('name', NAMES)
def test_the_option_arms_the_5x5_pairs_and_nothing_else(name):
    from metrabs_amd import backbones
    plain = fold(_net(name), torch.bfloat16, ())
    armed = fold(_net(name), torch.bfloat16, (NEW,))
    assert not _armed(plain, 'hand_k5_to') and not any('hand_k5_to' in m.__dict__ for m in plain.modules())
    pairs = _armed(armed, 'hand_k5_to')
    assert len(pairs) == PAIRS[name]
    # the three sibling fields are untouched by the new option, and hand_k5_to by theirs
    for option, field in SIBLINGS.items():
        assert not _armed(armed, field), field
        theirs = fold(_net(name), torch.bfloat16, (option,))
        assert not _armed(theirs, 'hand_k5_to'), option
        both = fold(_net(name), torch.bfloat16, (option, NEW))
        assert [n for n, _, _ in _armed(both, field)] == [n for n, _, _ in _armed(theirs, field)], option
        assert [n for n, _, _ in _armed(both, 'hand_k5_to')] == [n for n, _, _ in pairs], option
    # the same state_dict -- keys and tensors --, modules and buffers
    sp, sa = plain.state_dict(), armed.state_dict()
    assert list(sp) == list(sa) and all(torch.equal(sp[k], sa[k]) for k in sp)
    assert [(n, type(m)) for n, m in armed.named_modules()] == [(n, type(m)) for n, m in plain.named_modules()]
    assert [n for n, _ in armed.named_buffers()] == [n for n, _ in plain.named_buffers()]
    mods = dict(armed.named_modules())
    for n, e, d in pairs:
        assert n.endswith('.block.0.0') and mods[n[:-len('0.0')] + '1.0'] is d, n
        assert type(e) is backbones.ConvBiasAct and isinstance(d, backbones.DepthwiseBiasAct)
        assert (d.k, d.pad, d.pads) == (5, 2, None) and d.stride in (1, 2) and not e.emit_mean
        assert d.weight.shape[0] == e.conv.out_channels
    if name == 'mobilenetv3':
        assert sorted((e.conv.in_channels, e.conv.out_channels, d.stride) for _, e, d in pairs) == \
            [(24, 72, 2), (40, 120, 1), (40, 120, 1), (112, 672, 2), (160, 960, 1), (160, 960, 1)]
        assert all(d.emit_mean for _, _, d in pairs)
    # every 5x5 depthwise layer the option leaves alone has a folded padding or no plain 1x1 expand in front
    armed_dw = {id(d) for _, _, d in pairs}
    for m in armed.modules():
        if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 5:
            assert id(m) in armed_dw or m.pads is not None, name
    everything = fold(_net(name), torch.bfloat16, H16_OPTS + tuple(SIBLINGS) + (NEW,))
    assert stale_references(everything) == []
    assert len(_armed(everything, 'hand_k5_to')) == PAIRS[name]
    assert list(everything.state_dict()) == list(sp)


@pytest.mark.parametrize('name', NAMES)
def test_the_armed_copy_on_the_cpu_runs_the_chain(name):
    plain, armed = fold(_net(name), torch.bfloat16, ()), fold(_net(name), torch.bfloat16, (NEW,))
    x = torch.rand(2, 3, 96, 96, generator=torch.Generator().manual_seed(2))
    with torch.inference_mode():
        a, p = armed(x), plain(x)
    assert a.dtype == torch.bfloat16 and torch.isfinite(a.float()).all()
    assert torch.equal(a, p)
    assert [getattr(m, 'last_path', None) for m in armed.modules()] == [getattr(m, 'last_path', None)
                                                                       for m in plain.modules()]
    assert not any(getattr(m, 'last_path', None) == 'k28h' for m in armed.modules())


def test_the_kernels_use_no_scratch_and_leave_room_for_two_workgroups():
    """tests/test_kernel_resources.py walks every source of the library, this one included; here the new file's own
    instantiations (two dtypes, two strides, two slice widths) by name: no scratch, no spilled VGPR, no static LDS, and
    at most 256 registers -- two workgroups of four waves per CU, which the 80 KiB rule of the slice width counts on."""
    from metrabs_amd import build
    assert 'expand_dw16_k5.hip' in build.sources()
    ks = [k for k in build.kernel_resources('expand_dw16_k5.hip') if 'expand_dw16_k5_kernel' in k['name']]
    assert len(ks) == 8
    for k in ks:
        assert k['private_segment_fixed_size'] == 0 and k['vgpr_spill_count'] == 0, k
        assert k['group_segment_fixed_size'] == 0, k   # (all of its LDS is dynamic: the query's answer)
        assert k['vgpr_count'] <= 256, k
