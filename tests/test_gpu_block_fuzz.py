"""GPU: single MBConv, FusedMBConv and MBv3Block blocks with DRAWN channel counts, maps and options, folded and run on
their own (an nn.Sequential around one block is all fold_batchnorm needs: no option asks for more of a network).  The
dispatch in backbones.py is otherwise exercised on the shipped networks alone, whose channels are multiples of 8 and
whose maps are square.

12 blocks from random.Random(a fixed seed): the three block types in turn; channels multiples of 8 in a third of the
draws, multiples of 4 only in a third, odd in a third (every type meets every class); kernel size 3 or 5, stride,
bottomright, squeeze-excite on or off and both activations where the type has them; maps from 5 x 7 to 24 x 20, half of
them with the even height and the width of a multiple of 8 that the vector kernels ask for; B 1 .. 3; random batch-norm
statistics.  Each block is folded with every option of its family on (f32: F32_OPTS, f16 and bf16: H16_OPTS of
tests/test_backbone_option_combos_host.py), and once more as the default f32 copy, where K13 runs what split_gemm
hands to K20 in the armed one.  Asserted per block: the forward does not raise; every folded layer's last_path is what
the kernels.*_supported predicate of its kernel and its kernel_for answer for the tensor it was given ('library' where
the kernel refuses); f32 accuracy against an fp64 CPU forward of the same folded block (at most 2 x the error of the
block with every hand-written kernel off: DESIGN.md section 22's margin); the 16-bit criteria of
test_all_on_16bit_copy_meets_the_default_copys_criteria, factors unchanged.  Over the 12 draws every hand-written
kernel family shows up.  One BLOCK_FUZZ line per case."""
import copy
import random

import pytest
import torch
from torch import nn

from test_backbone_option_combos_host import F32_OPTS, H16_OPTS, fold
from test_gpu_conv1x1_split import _pinned

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
N_BLOCKS = 12
SEEN = {}   # case -> the set of last_path values of its copies (the last test reads it)


def _channels(rng, cls, lo, hi):
    """A channel count of class 0 (a multiple of 8), 1 (a multiple of 4 and not of 8) or 2 (odd) in lo .. hi."""
    pool = [c for c in range(lo, hi + 1) if (c % 8 == 0, c % 8 == 4, c % 2 == 1)[cls]]
    return rng.choice(pool)


def _draw_blocks():
    rng = random.Random(2929)
    blocks = []
    balanced = lambda n: rng.sample([False, True] * (n // 2), n)   # both values, as often as each other
    se, hs, bottomright, five = balanced(4), balanced(4), balanced(N_BLOCKS), balanced(N_BLOCKS)
    for i in range(N_BLOCKS):
        kind, cls = ('mbconv', 'fused', 'mbv3')[i % 3], (i + i // 3) % 3
        stride = 1 if i == 7 else rng.choice([1, 2])
        same = stride == 1 and rng.random() < 0.5          # cout == cin: the block has a skip
        cin = _channels(rng, cls, 5, 64)
        cout = cin if same else _channels(rng, cls, 5, 96)
        if i % 2 == 1:   # what the vector kernels ask of a map: H even, W a multiple of 8
            H, W = 2 * rng.randint(3, 12), 8 * rng.randint(1, 2)
        else:            # 5 x 7 .. 24 x 20, no constraint
            H, W = rng.randint(5, 24), rng.randint(7, 20)
        b = dict(kind=kind, cin=cin, cout=cout, stride=stride, H=H, W=W, B=rng.randint(1, 3), k=5 if five[i] else 3,
                 bottomright=bottomright[i] and i != 7, se=se[i // 3], hs=hs[i // 3])
        if kind == 'mbconv':
            b['expand'] = rng.choice([1, 4, 6])
        elif kind == 'fused':
            b['expand'], b['k'] = (4 if i == 7 else rng.choice([1, 4])), 3
        else:
            b['exp'] = cin if rng.random() < 0.25 else _channels(rng, cls, 8, 240)
        blocks.append(b)
    return blocks


BLOCKS = _draw_blocks()


def test_the_draws_are_what_the_module_says():
    assert [b['kind'] for b in BLOCKS] == ['mbconv', 'fused', 'mbv3'] * 4
    for kind in ('mbconv', 'fused', 'mbv3'):
        mine = [b for b in BLOCKS if b['kind'] == kind]
        assert {(b['cin'] % 8 == 0, b['cin'] % 8 == 4, b['cin'] % 2 == 1).index(True) for b in mine} == {0, 1, 2}
    for cls in (lambda c: c % 8 == 0, lambda c: c % 8 == 4, lambda c: c % 2 == 1):
        assert sum(cls(b['cin']) and cls(b['cout']) for b in BLOCKS) == 4
    assert all(5 <= b['H'] <= 24 and 7 <= b['W'] <= 20 and 1 <= b['B'] <= 3 for b in BLOCKS)
    assert {b['stride'] for b in BLOCKS} == {1, 2} and {b['k'] for b in BLOCKS} == {3, 5}
    assert {b['hs'] for b in BLOCKS if b['kind'] == 'mbv3'} == {False, True}
    assert {b['se'] for b in BLOCKS if b['kind'] == 'mbv3'} == {False, True}
    assert {b['bottomright'] for b in BLOCKS} == {False, True}
    assert sum(b['H'] % 2 == 1 or b['W'] % 4 != 0 for b in BLOCKS) >= 4   # odd maps: the library and scalar paths
    seven = BLOCKS[7]   # the one FusedMBConv with channels of a multiple of 8: K16h's
    assert seven['kind'] == 'fused' and seven['cin'] % 8 == 0 and seven['expand'] == 4 and seven['W'] % 8 == 0


def _build(b):
    from metrabs_amd import backbones
    torch.manual_seed(100 + BLOCKS.index(b))
    if b['kind'] == 'mbconv':
        blk = backbones.MBConv(b['cin'], b['cout'], b['expand'], b['stride'], k=b['k'], bottomright=b['bottomright'])
    elif b['kind'] == 'fused':
        blk = backbones.FusedMBConv(b['cin'], b['cout'], b['expand'], b['stride'], bottomright=b['bottomright'])
    else:
        blk = backbones.MBv3Block(b['cin'], b['k'], b['exp'], b['cout'], b['se'], b['hs'], b['stride'])
    for m in blk.modules():   # random statistics: a folded batch norm that is no identity
        if isinstance(m, nn.BatchNorm2d):
            m.running_mean.normal_(0, 0.1)
            m.running_var.uniform_(0.5, 1.5)
            m.weight.data.uniform_(0.5, 1.5)
            m.bias.data.normal_(0, 0.1)
    return nn.Sequential(blk).eval().cuda()


def _expected(m, x, kw):
    """The last_path of a folded layer for the call it received, from the predicate of its kernel and its kernel_for."""
    from metrabs_amd import backbones as B, kernels
    if isinstance(m, B.DepthwiseBiasAct):
        pad = (m.pad,) * 4 if m.pads is None else m.pads
        ow = (x.shape[3] + pad[0] + pad[1] - m.k) // m.stride + 1
        if ow % 4:
            return ['library']
        if m.k == 5:
            return ['k15' if kernels.depthwise5x5_supported(x.shape[2], x.shape[3], pad) else 'library']
        k18 = m.block_depthwise and m.pads is None and not kernels.k11_takes_block_kernel(x.shape[2], x.shape[3]) \
            and kernels.depthwise3x3_blocks_supported(x.dtype, x.shape[2], x.shape[3], m.stride, m.pad, x.data_ptr())
        return ['k18' if k18 else 'k11']
    w = m.conv.weight
    xc = x.to(w.dtype) if x.dtype != w.dtype and w.dtype in (F16, BF16) else x
    r = kw.get('residual')
    if kw.get('defer_epilogue') or (r is not None and (r.dtype != xc.dtype or not r.is_contiguous()
                                                       or r.data_ptr() % 16)):
        return ['library']   # (a skip no epilogue can add: _addable)
    if isinstance(m, B.Conv3x3BiasAct):
        return ['k14h' if kernels.conv3x3_16_supported(xc, m.weight_packed, m.stride) else 'library']
    if isinstance(m, B.WinogradConv3x3BiasAct) and kw.get('pre') is None and \
            kernels.conv3x3_winograd_supported(xc, kernels.pack_conv3x3_winograd_weight(w)):
        return ['k19']
    if m.conv.kernel_size != (1, 1):
        return ['library']
    ok = kernels.conv1x1_supported(xc, w) if xc.dtype == torch.float32 else kernels.conv1x1_16_supported(xc, w)
    kernel = m.kernel_for(xc)
    assert (kernel is not None) == ok, (kernel, ok, tuple(xc.shape))
    if kernel is None:
        return ['library']
    assert kernel in (('k20', 'k13') if xc.dtype == torch.float32 else ('k13h', 'k13h_deep'))
    assert kernel != 'k20' or m.split_gemm
    return [kernel, kernel + '_gate']


def _forward(net, x):
    """One forward -> (output, [(layer, the path it reported, the paths it may report)], every last_path)."""
    from metrabs_amd import backbones as B
    layers = [m for m in net.modules() if isinstance(m, (B.ConvBiasAct, B.Conv3x3BiasAct, B.DepthwiseBiasAct))]
    calls, hooks = {}, []
    for m in layers:
        hooks.append(m.register_forward_pre_hook(
            lambda mod, args, kwargs: calls.__setitem__(mod, (args[0], dict(kwargs))), with_kwargs=True))
    try:
        with torch.inference_mode(), _pinned():
            y = net(x).clone()
            report = [(m, m.last_path, _expected(m, *calls[m])) for m in layers if m in calls]
    finally:
        for h in hooks:
            h.remove()
    # every folded layer ran, or the block ran as one launch in their place (K16h)
    assert len(calls) == len(layers) or any(getattr(m, 'last_path', None) == 'k16h' for m in net.modules())
    return y, report, [p for p in (getattr(m, 'last_path', None) for m in net.modules()) if p is not None]


def _rel_rms(y, want):
    return float((y.double().cpu() - want).norm() / want.norm())


@pytest.mark.parametrize('i', range(N_BLOCKS))
def test_block(i, hip_lib):
    from metrabs_amd import backbones
    b = BLOCKS[i]
    net = _build(b)
    x = torch.randn(b['B'], b['cin'], b['H'], b['W'], device='cuda',
                    generator=torch.Generator(device='cuda').manual_seed(500 + i))
    # multiples of 1 / 16 below 8: exact in f32, f16 and bf16, so no copy is charged with rounding its input
    x = (x.clamp(-7.9, 7.9) * 16).round() / 16
    assert torch.equal(x.half().float(), x) and torch.equal(x.bfloat16().float(), x)
    off = backbones.fold_batchnorm(net)                       # no hand-written kernel: the torch ops alone
    copies = {'f32': fold(net, None, ()), 'f32_all': fold(net, None, F32_OPTS), 'f16_all': fold(net, F16, H16_OPTS),
              'bf16_all': fold(net, BF16, H16_OPTS)}
    with torch.inference_mode(), _pinned():
        y_off = off(x).clone()
        want = copy.deepcopy(off).cpu().double()(x.double().cpu())
    out, paths = {}, set()
    for key, net_c in copies.items():
        # a block of a 16-bit copy receives the copy's dtype (the network's first convolution casts, once): with an f32
        # input the skip would be f32 beside a 16-bit result, which no epilogue adds and torch promotes to f32
        dtype = getattr(net_c, 'inference_dtype', torch.float32)
        out[key], report, every = _forward(net_c, x.to(dtype))
        paths |= set(every)
        for m, got, may in report:
            assert got in may, (key, type(m).__name__, got, may, b)
        assert torch.isfinite(out[key].float()).all() and out[key].shape == want.shape
    SEEN[i] = paths
    # f32: against fp64, relative to the block with every hand-written kernel off
    e_off, e_f32, e_all = _rel_rms(y_off, want), _rel_rms(out['f32'], want), _rel_rms(out['f32_all'], want)
    # 16-bit: against the f32 folded block, relative to that block under autocast
    a = out['f32'].float()
    amax = float(a.abs().max())
    line = f'BLOCK_FUZZ {i} {b}: paths {sorted(paths)}; f32 rel RMS vs fp64 off {e_off:.3g} default {e_f32:.3g} all-on {e_all:.3g}'
    stats = {}
    for dtype, key in ((F16, 'f16_all'), (BF16, 'bf16_all')):
        # (under autocast, too, a block inside a network is handed the 16-bit result of the layer in front: its skip and
        # its depthwise layer then work in 16 bits as the copy's do, and its result is a 16-bit tensor like the copy's)
        with torch.inference_mode(), _pinned(), torch.autocast('cuda', dtype=dtype):
            auto = copies['f32'](x.to(dtype))
        assert auto.dtype == dtype
        auto = auto.float()
        c = out[key].float()
        stats[key] = (float((c - a).abs().mean()), float((auto - a).abs().mean()), float((c - a).abs().max()),
                      float((auto - a).abs().max()))
        line += f'; {key} mean-abs {stats[key][0]:.3g} (autocast {stats[key][1]:.3g}) max-abs {stats[key][2]:.3g} ' \
                f'(autocast {stats[key][3]:.3g})'
    print(line + f'; amax {amax:.3g}')
    assert e_f32 <= 2 * e_off and e_all <= 2 * e_off, (e_off, e_f32, e_all)
    for key, (mean_c, mean_b, max_c, max_b) in stats.items():
        assert out[key].dtype == (F16 if key == 'f16_all' else BF16)
        assert mean_c <= 1.1 * mean_b + 1e-6 * amax, (key, mean_c, mean_b)
        if max_b <= 0.1 * amax:
            assert max_c <= 0.1 * amax, (key, max_c, max_b, amax)
        else:
            assert max_c <= 1.1 * max_b, (key, max_c, max_b, amax)


def test_every_kernel_family_ran_somewhere_over_the_draws(hip_lib):
    assert sorted(SEEN) == list(range(N_BLOCKS)), 'runs behind test_block, in one process'
    union = set().union(*SEEN.values())
    base = {p[:-len('_gate')] if p.endswith('_gate') else p for p in union}
    for family in (('k11', 'k18'), ('k13', 'k13_pre'), ('k13h', 'k13h_deep'), ('k16h',), ('k19', 'k22'),
                   ('k20', 'k20_pre')):
        assert base & set(family), (family, sorted(union))
    assert 'library' in union   # and the refusals
