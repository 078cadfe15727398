"""Plain-torch.nn restatements of the reference's backbones, random-initialised, for the synthetic
benchmark workloads of BASELINE.json (torchvision is not in this image and there is no network for
checkpoints).  The networks as built here run on PyTorch-ROCm (MIOpen / rocBLAS); the inference copy that
fold_batchnorm makes of one is part of the hand-written hot path: its folded layers (ConvBiasAct and the classes beside
it, below) run the HIP kernels K10 to K20 of kernels.py wherever one takes the tensor, and the library everywhere else.
Each folded layer decides that once per forward, in its path().  Only the output shape matters
to what follows: [B, C, P/32, P/32] with C = 1280 (EffNetV2-S/L, MobileNetV3-L) or 512 (ResNet-18).

Architecture tables follow metrabs_pytorch/backbones/efficientnet.py:379-435 (EfficientNetV2 S/L:
FusedMBConv/MBConv stages, SE ratio 0.25, BN eps 1e-3, PreprocLayer x*2-1 :1181-1186),
metrabs_tf/backbones/resnet.py:746-754 (ResNet-18) and metrabs_tf/backbones/mobilenet_v3.py:387-432
(MobileNetV3-Large, last_point_ch 1280).  Padding is symmetric k//2 (the reference uses TF-'SAME'
fixed padding, efficientnet.py:1127-1161; irrelevant for throughput).
"""
import collections
import threading

import torch
import torch.nn.functional as F
from torch import nn

from . import _lib, kernels


class DepthwiseConv2d(nn.Conv2d):
    """A depthwise convolution that runs on PyTorch's own HIP depthwise kernel instead of MIOpen.
    MIOpen serves f32 / f16 NCHW depthwise 3x3 with its naive direct kernel on this stack; with
    MIOpen switched off for these layers the EfficientNetV2-S forward at the bench shape takes
    13.13 instead of 14.02 ms in f32 (10.87 vs 11.71 ms under f16 autocast), features equal to
    5e-6 relative (tools/experiments/depthwise_backend_probe.py).  Same parameters, same
    state_dict keys; still PyTorch-ROCm, only the backend choice of these layers changes."""

    use_miopen = False  # class-wide switch (tools/experiments/depthwise_backend_probe.py flips it)
    _backend_lock = threading.Lock()  # the MIOpen switch is process-global state in torch

    def forward(self, x):
        if x.is_cuda and not DepthwiseConv2d.use_miopen and torch.backends.cudnn.enabled:
            # scoped; the lock serialises THESE layers among themselves (two of them must not
            # interleave their save / restore of the flag).  It does not isolate other threads'
            # convolutions: a convolution another thread launches while this context is open sees
            # MIOpen off too (the switch is process-global in torch).  Every other flag is passed
            # through unchanged -- flags() would otherwise reset benchmark / deterministic /
            # allow_tf32 to its keyword defaults inside the context.
            cudnn = torch.backends.cudnn
            with DepthwiseConv2d._backend_lock, cudnn.flags(
                    enabled=False, benchmark=cudnn.benchmark, deterministic=cudnn.deterministic,
                    allow_tf32=cudnn.allow_tf32):
                return super().forward(x)
        return super().forward(x)


class ConvBNAct(nn.Sequential):
    """conv '0' + batch norm '1' (+ activation '2'): the parameter names of torchvision's
    Conv2dNormActivation, which the reference's checkpoints use."""

    def __init__(self, cin, cout, k=3, s=1, groups=1, act=nn.SiLU, eps=1e-3, padding=None):
        conv = DepthwiseConv2d if groups == cin == cout and groups > 1 else nn.Conv2d
        layers = [conv(cin, cout, k, s, k // 2 if padding is None else padding, groups=groups,
                       bias=False),
                  nn.BatchNorm2d(cout, eps=eps)]
        if act is not None:
            layers.append(act())
        super().__init__(*layers)


class SqueezeExcite(nn.Module):
    def __init__(self, channels, squeeze, gate=nn.Sigmoid, act=nn.SiLU):
        super().__init__()
        self.fc1 = nn.Conv2d(channels, squeeze, 1)
        self.fc2 = nn.Conv2d(squeeze, channels, 1)
        self.act, self.gate = act(), gate()

    # set by fold_batchnorm(fused_epilogue=True): the ConvBiasAct in front of this block, whose
    # epilogue pass also produced the per-channel mean of the tensor it handed over
    mean_from = ()
    # set by fold_batchnorm(fused_epilogue=True): the ConvBiasAct of the block's project conv, which
    # applies the gate to its input itself where one of its 1x1 kernels takes the tensor (ConvBiasAct.applies_gate)
    gate_to = ()

    _GATE_NAMES = {nn.Sigmoid: 'sigmoid', nn.Hardsigmoid: 'hardsigmoid'}

    def forward(self, x):
        mean = None
        for src in self.mean_from:
            mean = src.take_mean_f32(x)
        if mean is not None and self._fused_gate_ok():
            # fc1, + b1, act, fc2, + b2, gate as ONE HIP launch from the f32 mean (K12)
            g = kernels.se_gate(mean, self.fc1.weight, self.fc1.bias, self.fc2.weight, self.fc2.bias,
                                _ACT_NAMES[type(self.act)], self._GATE_NAMES[type(self.gate)], w2t=self._fc2_wt())
            for dst in self.gate_to:
                if dst.applies_gate(x):
                    # the project conv multiplies x by the gate as it stages x: no x * g pass
                    dst.give_gate(x, g)
                    return x
            return x * g.to(x.dtype).view(x.shape[0], x.shape[1], 1, 1)
        if x.dtype != self.fc1.weight.dtype and _autocast_off(x.device.type):
            return self._forward_16bit_copy(x, mean)
        s = None if mean is None else mean.to(x.dtype).view(x.shape[0], x.shape[1], 1, 1)
        if s is None:
            s = x.mean((2, 3), keepdim=True)
        return x * self.gate(self.fc2(self.act(self.fc1(s))))

    def _forward_16bit_copy(self, x, mean):
        """The unfused block in a 16-bit copy (fold_batchnorm(dtype=)): its parameters stay f32, so does its
        arithmetic, from the f32 mean (the epilogue's, or one taken here); x * gate in x's dtype."""
        s = mean.view(x.shape[0], x.shape[1], 1, 1) if mean is not None else \
            x.mean((2, 3), keepdim=True, dtype=self.fc1.weight.dtype)
        return x * self.gate(self.fc2(self.act(self.fc1(s)))).to(x.dtype)

    _w2t = None

    def _fc2_wt(self):
        """fc2's weight transposed to [S, C] for K12 (a wave's fc2 loads are then contiguous): made on the first
        fused forward and kept as _derived_weight says."""
        self._w2t = _derived_weight(self._w2t, self.fc2.weight,
                                    lambda w: w.detach().reshape(w.shape[0], -1).t().contiguous())
        return self._w2t[1]

    def _fused_gate_ok(self):
        """K12 computes no gradient: only where none is wanted, for the layer types it implements."""
        return (_no_grad_wanted(self.parameters())
                and type(self.act) in (nn.SiLU, nn.ReLU) and type(self.gate) in self._GATE_NAMES
                and self.fc1.weight.dtype == torch.float32 and self.fc1.bias is not None
                and self.fc2.bias is not None and self.fc1.weight.is_cuda
                and self.fc1.in_channels % 4 == 0)


def _padded_conv(layers, name, cin, cout, k, stride, groups=1, act=nn.SiLU, bottomright=False):
    """The reference pads explicitly (TF 'SAME' independent of the input size,
    efficientnet.py:1127-1161: (k-1)//2 before, the rest after, shifted one pixel to the bottom
    right for the `bottomright_stride` layer) and convolves unpadded.  Symmetric padding is folded
    into the convolution (same zeros, one op less); the asymmetric case keeps a ZeroPad2d, which
    has no parameters, so the checkpoint keys are unaffected either way."""
    total = k - 1
    beg, end = total // 2, total - total // 2
    if bottomright:
        layers['padding'] = nn.ZeroPad2d((beg - 1, end + 1, beg - 1, end + 1))
        layers[name] = ConvBNAct(cin, cout, k, stride, groups=groups, act=act, padding=0)
    elif beg == end:
        layers[name] = ConvBNAct(cin, cout, k, stride, groups=groups, act=act, padding=beg)
    else:
        layers['padding'] = nn.ZeroPad2d((beg, end, beg, end))
        layers[name] = ConvBNAct(cin, cout, k, stride, groups=groups, act=act, padding=0)


class FusedMBConv(nn.Module):
    """efficientnet.py:176-234 (module names '0' [, '1'] inside `block`)."""

    def __init__(self, cin, cout, expand, stride, bottomright=False):
        super().__init__()
        self.residual = stride == 1 and cin == cout
        mid = cin * expand
        layers = collections.OrderedDict()
        if expand == 1:
            _padded_conv(layers, '0', cin, cout, 3, stride, bottomright=bottomright)
        else:
            _padded_conv(layers, '0', cin, mid, 3, stride, bottomright=bottomright)
            layers['1'] = ConvBNAct(mid, cout, 1, 1, act=None)
        self.block = nn.Sequential(layers)

    # set by fold_batchnorm(fuse_blocks=True) on a 16-bit copy: (the block's Conv3x3BiasAct, its project
    # ConvBiasAct) -- references, as SqueezeExcite.mean_from: nothing is registered twice, no weight is copied
    fused_pair = ()
    # 'k16h' / 'k13_pre' / 'k20_pre' / 'k19' / 'k21' / 'k22' or 'chain': what the last forward of an armed block ran (tests, A/B runs); None on
    # every other block
    last_path = None
    # class-wide switch (tests and A/B runs): the two-kernel chain everywhere
    use_k16h = True
    # (Cin, Cmid, Cout, stride, H, W) of the input where K16h measured slower than the chain as the default copy
    # runs it in f16 or bf16, both timed as HIP graph replays
    k16h_slower = frozenset()

    def k16h_takes(self, x):
        """Whether forward(x) runs the armed block as one launch (K16h, fused_mbconv16.hip): a CUDA NCHW-contiguous
        input of the copy's dtype, autocast off, no gradient wanted, a shape the C entry accepts and that is not
        listed as slower."""
        if not (self.fused_pair and FusedMBConv.use_k16h and x.is_cuda and x.dim() == 4):
            return False
        expand, project = self.fused_pair
        w3, w1 = expand.conv.weight, project.conv.weight
        if x.dtype != w3.dtype or w1.dtype != w3.dtype or x.dtype not in (torch.float16, torch.bfloat16):
            return False
        if not _inference_call(w3, w1):
            return False
        if (w3.shape[1], w3.shape[0], w1.shape[0], expand.stride, x.shape[2], x.shape[3]) in FusedMBConv.k16h_slower:
            return False
        return kernels.fused_mbconv16_supported(x, expand.weight_packed, w1, expand.stride)

    # set by fold_batchnorm(fused_epilogue=True) on an f32 copy: (the block's 3x3 ConvBiasAct, its project
    # ConvBiasAct) -- references, like fused_pair.  The 3x3 layer's K10 pass ("+ bias", activation) is left out and
    # applied by the project's K13 launch to every element on its way into the GEMM: the same bits, one read and one
    # write of the expanded activation less
    pre_pair = ()
    # class-wide switch (tests and A/B runs): K10 behind the 3x3 convolution everywhere
    use_k13_pre = True
    # (Cin, Cmid, Cout, stride, H, W) of the input where K13 with the prologue measured slower than K10 + K13 as HIP
    # graph replays: these stay on the chain
    k13_pre_slower = frozenset()

    def _forward_pre(self, x):
        """An armed f32 block.  'k13_pre': the 3x3 convolution alone, then ONE K13 launch that applies its epilogue,
        the project and the skip; 'k20_pre': the same launch on K20, where fold_batchnorm(split_gemm=True) armed the
        project and K20 takes the tensor.  'k21' / 'k19' / 'k22' (a Dense3x3BiasAct first layer, from
        fold_batchnorm(split3x3 / winograd3x3 / strided3x3=True), that says so): the 3x3 convolution WITH its epilogue
        on that kernel of DENSE3X3_KERNELS, then the project and the skip as an ordinary call of the project layer --
        K13, or K20 under split_gemm (the project's own last_path says which).  With the kernel switched off or
        refusing, such a layer is the ConvBiasAct it derives from, and the block takes the other branches.  'chain':
        what an unarmed block runs.  The block asks the layers (path(), last_path) and decides
        nothing for them; the tensor without its epilogue goes to the project alone, which applies that epilogue on
        every path, and no tensor passes through two epilogues.  (tests/test_gpu_backbone_option_combos.py runs the
        branches with every option on.)"""
        first, project = self.pre_pair
        c = first.conv
        residual = x if self.residual else None
        first_path = first.path(x) if isinstance(first, Dense3x3BiasAct) else None
        if first_path in DENSE3X3_KERNELS:
            # the kernel applies the 3x3 layer's own epilogue; the project is then an ordinary call (K13, or K20 under
            # split_gemm; no prologue) with the skip
            self.last_path = first_path
            return project(first(x), residual=residual)
        self.last_path = 'chain'
        if not (FusedMBConv.use_k13_pre and x.is_cuda and x.dim() == 4 and x.dtype == torch.float32
                and c.weight.dtype == torch.float32 and _inference_call(c.weight, x=x)
                and (c.in_channels, c.out_channels, project.conv.out_channels, c.stride[0], x.shape[2], x.shape[3])
                not in FusedMBConv.k13_pre_slower):
            return _block_plus_skip(self.block, x) if self.residual else self.block(x)
        y = project(first(x, defer_epilogue=True), residual=residual, pre=first)
        # (fold_batchnorm(split_gemm=True): the same launch on K20 where it takes the tensor; a project that refuses
        # ran K10 and its own library path: the chain)
        self.last_path = {'k13': 'k13_pre', 'k20': 'k20_pre'}.get(project.last_path, 'chain')
        return y

    def forward(self, x):
        if self.pre_pair:
            return self._forward_pre(x)
        if self.fused_pair:
            if self.k16h_takes(x):
                expand, project = self.fused_pair
                self.last_path = 'k16h'
                return kernels.fused_mbconv16(x, expand.weight_packed, expand.bias, expand.act_name, expand.stride,
                                              project.conv.weight, project.bias,
                                              residual=x if self.residual else None)
            self.last_path = 'chain'
        return _block_plus_skip(self.block, x) if self.residual else self.block(x)


class MBConv(nn.Module):
    """efficientnet.py:110-173: '0' expand 1x1, '1' depthwise, '2' squeeze-excite (fc1, fc2),
    '3' project."""

    def __init__(self, cin, cout, expand, stride, k=3, bottomright=False):
        super().__init__()
        self.residual = stride == 1 and cin == cout
        mid = cin * expand
        layers = collections.OrderedDict()
        if mid != cin:
            layers['0'] = ConvBNAct(cin, mid, 1, 1)
        n = len(layers)
        _padded_conv(layers, str(n), mid, mid, k, stride, groups=mid, bottomright=bottomright)
        layers[str(n + 1)] = SqueezeExcite(mid, max(1, cin // 4))
        layers[str(n + 2)] = ConvBNAct(mid, cout, 1, 1, act=None)
        self.block = nn.Sequential(layers)

    def forward(self, x):
        return _block_plus_skip(self.block, x) if self.residual else self.block(x)


class Preproc(nn.Module):
    """PreprocLayer (efficientnet.py:1181-1186): [0,1] -> [-1,1]."""

    # set by fold_batchnorm(fuse_stem=True): the StemConvBiasAct directly behind this layer, which applies
    # x * 2 - 1 itself as it stages x (K17) -- a reference, as SqueezeExcite.mean_from: nothing is registered twice
    hand_to = ()

    def forward(self, x):
        for dst in self.hand_to:
            if dst.k17_takes(x):
                # decided here, once: the stem convolution reads x in place and applies Preproc on the way in
                dst.hand_over(x)
                return x
        return x * 2 - 1


EFFNETV2 = {
    # (block, expand, stride, cin, cout, n_layers); efficientnet.py:399-431.  The LAST stride-2 stage
    # is the `bottomright_stride=FLAGS.centered_stride` one.
    's': dict(stem=24, stages=[('f', 1, 1, 24, 24, 2), ('f', 4, 2, 24, 48, 4), ('f', 4, 2, 48, 64, 4),
                               ('m', 4, 2, 64, 128, 6), ('m', 6, 1, 128, 160, 9),
                               ('m', 6, 2, 160, 256, 15)], head=1280),
    'm': dict(stem=24, stages=[('f', 1, 1, 24, 24, 3), ('f', 4, 2, 24, 48, 5), ('f', 4, 2, 48, 80, 5),
                               ('m', 4, 2, 80, 160, 7), ('m', 6, 1, 160, 176, 14),
                               ('m', 6, 2, 176, 304, 18), ('m', 6, 1, 304, 512, 5)], head=1280),
    'l': dict(stem=32, stages=[('f', 1, 1, 32, 32, 4), ('f', 4, 2, 32, 64, 7), ('f', 4, 2, 64, 96, 7),
                               ('m', 4, 2, 96, 192, 10), ('m', 6, 1, 192, 224, 19),
                               ('m', 6, 2, 224, 384, 25), ('m', 6, 1, 384, 640, 7)], head=1280),
}


def efficientnetv2(size='s', centered_stride=True):
    """`Sequential(PreprocLayer(), efficientnet_v2_<size>().features)` of the reference
    (scripts/demo_image.py:63-66) with the same module tree, hence the same state_dict keys
    ('1.0.0.weight' = stem conv, '1.<stage>.<i>.block.<k>....', '1.<last>.0.weight' = 1x1 head conv)
    and the same arithmetic (checked against the reference's own class on shared weights,
    tests/test_oracle_pin.py)."""
    cfg = EFFNETV2[size]
    feats = collections.OrderedDict()
    _padded_conv(feats, '0', 3, cfg['stem'], 3, 2)
    last_s2 = max(i for i, st in enumerate(cfg['stages']) if st[2] == 2)
    for si, (kind, expand, stride, cin, cout, n) in enumerate(cfg['stages']):
        blk = FusedMBConv if kind == 'f' else MBConv
        stage = [blk(cin if i == 0 else cout, cout, expand, stride if i == 0 else 1,
                     bottomright=(centered_stride and si == last_s2 and i == 0)) for i in range(n)]
        feats[str(si + 1)] = nn.Sequential(*stage)
    feats[str(len(cfg['stages']) + 1)] = ConvBNAct(cfg['stages'][-1][4], cfg['head'], 1, 1)
    net = nn.Sequential(Preproc(), nn.Sequential(feats))
    net.out_channels = cfg['head']
    return net


class BasicBlock(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.a = ConvBNAct(cin, cout, 3, stride, act=nn.ReLU, eps=1e-5)
        self.b = ConvBNAct(cout, cout, 3, 1, act=None, eps=1e-5)
        self.down = None if stride == 1 and cin == cout else ConvBNAct(cin, cout, 1, stride, act=None, eps=1e-5)

    def forward(self, x):
        idt = x if self.down is None else self.down(x)
        return torch.relu(self.b(self.a(x)) + idt)


def resnet18():
    layers = [ConvBNAct(3, 64, 7, 2, act=nn.ReLU, eps=1e-5), nn.MaxPool2d(3, 2, 1)]
    cin = 64
    for cout, stride in [(64, 1), (128, 2), (256, 2), (512, 2)]:
        layers += [BasicBlock(cin, cout, stride), BasicBlock(cout, cout, 1)]
        cin = cout
    net = nn.Sequential(*layers)
    net.out_channels = 512
    return net


class MBv3Block(nn.Module):
    def __init__(self, cin, k, exp, cout, se, hs, stride):
        super().__init__()
        act = nn.Hardswish if hs else nn.ReLU
        self.residual = stride == 1 and cin == cout
        layers = []
        if exp != cin:
            layers.append(ConvBNAct(cin, exp, 1, 1, act=act))
        layers.append(ConvBNAct(exp, exp, k, stride, groups=exp, act=act))
        if se:
            layers.append(SqueezeExcite(exp, max(8, exp // 4), gate=nn.Hardsigmoid, act=nn.ReLU))
        layers.append(ConvBNAct(exp, cout, 1, 1, act=None))
        self.block = nn.Sequential(*layers)

    def forward(self, x):
        return _block_plus_skip(self.block, x) if self.residual else self.block(x)


def mobilenet_v3_large():
    table = [(3, 16, 16, 0, 0, 1), (3, 64, 24, 0, 0, 2), (3, 72, 24, 0, 0, 1), (5, 72, 40, 1, 0, 2),
             (5, 120, 40, 1, 0, 1), (5, 120, 40, 1, 0, 1), (3, 240, 80, 0, 1, 2), (3, 200, 80, 0, 1, 1),
             (3, 184, 80, 0, 1, 1), (3, 184, 80, 0, 1, 1), (3, 480, 112, 1, 1, 1), (3, 672, 112, 1, 1, 1),
             (5, 672, 160, 1, 1, 2), (5, 960, 160, 1, 1, 1), (5, 960, 160, 1, 1, 1)]
    layers = [Preproc(), ConvBNAct(3, 16, 3, 2, act=nn.Hardswish)]
    cin = 16
    for k, exp, cout, se, hs, s in table:
        layers.append(MBv3Block(cin, k, exp, cout, bool(se), bool(hs), s))
        cin = cout
    layers += [ConvBNAct(cin, 960, 1, 1, act=nn.Hardswish), ConvBNAct(960, 1280, 1, 1, act=nn.Hardswish)]
    net = nn.Sequential(*layers)
    net.out_channels = 1280
    return net


def build_backbone(name):
    name = name.lower()
    if name in ('efficientnetv2-s', 'effnetv2-s', 'effv2s'):
        return efficientnetv2('s')
    if name in ('efficientnetv2-l', 'effnetv2-l', 'effv2l'):
        return efficientnetv2('l')
    if name in ('resnet18', 'resnet-18'):
        return resnet18()
    if name in ('mobilenetv3', 'mobilenetv3-large', 'mobilenet-v3'):
        return mobilenet_v3_large()
    raise ValueError(f'unknown backbone {name}')


_ACT_NAMES = {nn.SiLU: 'silu', nn.ReLU: 'relu', nn.Hardswish: 'hardswish'}
_16BIT = (torch.float16, torch.bfloat16)
_FLOATS = (torch.float32,) + _16BIT


# ---- what the folded layers below ask of a call, a convolution, a skip connection: each question written once

def _autocast_off(device_type='cuda'):
    return not torch.is_autocast_enabled(device_type)


def _no_grad_wanted(tensors):
    """No hand-written kernel computes a gradient: they run only where none is wanted for `tensors` (an iterable, looked
    at in grad mode alone)."""
    return not (torch.is_grad_enabled() and any(t.requires_grad for t in tensors))


def _inference_call(*weights, x=None):
    """An inference call: autocast off, and no gradient wanted for these weights -- nor for the input, where the caller
    passes it as `x` (K17, K19 and the K13 prologue do; K13, K13h, K14h, K16h and K20 look at their weights alone)."""
    return _autocast_off() and _no_grad_wanted(weights if x is None else weights + (x,))


def _plain_1x1(conv):
    """A plain 1x1 convolution: stride 1, unpadded, undilated, ungrouped, without a bias of its own (folded layers keep
    theirs beside the conv)."""
    return (conv.kernel_size == (1, 1) and conv.stride == (1, 1) and conv.padding == (0, 0) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.bias is None and conv.padding_mode == 'zeros')


def _dense_3x3(conv, strides):
    """A dense 3x3, padding-1 convolution with one of `strides`: what K14h, K17 and K19 are written for."""
    return (isinstance(conv, nn.Conv2d) and conv.groups == 1 and conv.kernel_size == (3, 3)
            and conv.dilation == (1, 1) and conv.stride in strides and conv.padding == (1, 1)
            and conv.padding_mode == 'zeros')


def _addable(residual, x, shape=None):
    """Whether a kernel's epilogue can add `residual` to a result like `x`: none at all, or x's dtype, contiguous and
    16-byte aligned -- and of `shape`, where the caller knows the result's (K19 does; the others leave the shape to
    the kernels.py wrapper, which raises)."""
    return residual is None or (residual.dtype == x.dtype and residual.is_contiguous()
                                and (shape is None or residual.shape == shape) and residual.data_ptr() % 16 == 0)


def _to_copy_dtype(x, weight):
    """The first convolution of a 16-bit copy casts its input, once: `x` in the dtype of `weight` (autocast off)."""
    if x.dtype != weight.dtype and weight.dtype in _16BIT and _autocast_off(x.device.type):
        return x.to(weight.dtype)
    return x


def _derived_weight(slot, w, make):
    """A tensor derived from the weight `w` (transposed, split, transformed: no part of the state dict), kept in a slot
    that is None or (key, tensor): -> the slot to keep, with make(w) made anew whenever the weight has moved or been
    written since.  An inference tensor carries no version counter: after writing such a weight in place, set the
    slot to None."""
    key = (w.data_ptr(), w.device, None if w.is_inference() else w._version)
    return slot if slot is not None and slot[0] == key else (key, make(w))


# The kernels that run the 1x1 expand of an MBConv block and the depthwise layer behind it (3x3; K28h: 5x5) as one
# launch, in the order an armed expand asks them (their planes, or their layers, are disjoint).  Per kernel, which is
# also its last_path: the fold_batchnorm option that arms the pairs, the ConvBiasAct field it sets on the expand (a field
# of its own per option, so no two options arm one field), DepthwiseBiasAct's question, class-wide switch and list of
# slower shapes, the wrapper in kernels, and what the call passes beside the tensors: the layer's stride (`strided`; the
# key of the slower list then carries it as a fifth element) and / or want_mean (`mean`).  THE place that says which goes
# with which.
EXPAND_DW_KERNELS = {
    'k25h': dict(option='fuse_expand_depthwise', field='hand_to', takes='k25h_takes', switch='use_k25h',
                 slower='k25h_slower', fn='expand_depthwise16', strided=False, mean=True),
    'k26h': dict(option='fuse_expand_depthwise_planes', field='hand_planes_to', takes='k26h_takes',
                 switch='use_k26h', slower='k26h_slower', fn='expand_depthwise16_planes', strided=False, mean=True),
    'k27h': dict(option='fuse_expand_depthwise_tiles', field='hand_tiles_to', takes='k27h_takes',
                 switch='use_k27h', slower='k27h_slower', fn='expand_depthwise16_tiles', strided=True, mean=False),
    'k28h': dict(option='fuse_expand_depthwise5x5', field='hand_k5_to', takes='k28h_takes', switch='use_k28h',
                 slower='k28h_slower', fn='expand_depthwise16_k5', strided=True, mean=True),
}

# The kernels that run a dense 3x3, padding-1 layer of an f32 copy with its epilogue as one launch, in the order a layer
# armed for several asks them (Dense3x3BiasAct.path): K21 in front of K19; K22's layers, of stride 2, are disjoint from
# both.  Per kernel, which is also its last_path: the fold_batchnorm option that replaces the layers, the class they
# become, which carries the class-wide switch and the list of slower shapes, the packer of the weight and the layer's
# attribute that keeps the packed weight (a _derived_weight slot, one per kernel), the C library's shape query and the
# wrapper in kernels, the layer's stride and what Cin must be a multiple of.  THE place that says which goes with which.
DENSE3X3_KERNELS = {
    'k21': dict(option='split3x3', cls='SplitConv3x3BiasAct', switch='use_k21', slower='k21_slower',
                pack='pack_conv3x3_split_weight', slot='_w3s', query='mtr_conv3x3_split_lds_bytes',
                fn='conv3x3_bias_act_split', stride=1, cin_multiple=8),
    'k19': dict(option='winograd3x3', cls='WinogradConv3x3BiasAct', switch='use_k19', slower='k19_slower',
                pack='pack_conv3x3_winograd_weight', slot='_wu', query='mtr_conv3x3_winograd_lds_bytes',
                fn='conv3x3_winograd_bias_act', stride=1, cin_multiple=4),
    'k22': dict(option='strided3x3', cls='StridedConv3x3BiasAct', switch='use_k22', slower='k22_slower',
                pack='pack_conv3x3_strided_weight', slot='_wsd', query='mtr_conv3x3s2_lds_bytes',
                fn='conv3x3_strided_bias_act', stride=2, cin_multiple=4),
}


class ConvBiasAct(nn.Module):
    """A folded conv + BN (+ activation): the convolution without its bias (MIOpen / rocBLAS), then
    "+ bias[c]" and the activation as ONE in-place pass (kernels.bias_act_, K10) instead of the two
    elementwise kernels PyTorch-ROCm would launch.  CPU tensors take the plain torch ops."""

    def __init__(self, conv, bias, act):
        super().__init__()
        self.conv = conv
        self.register_buffer('bias', bias.detach().float().contiguous())
        self.act = act
        self.act_name = None if act is None else _ACT_NAMES[type(act)]
        self.emit_mean = False  # a squeeze-excite block follows: give it its x.mean((2, 3)) for free
        self._mean = None
        self._gate = None
        # 'k13', 'k13_gate', 'k20', 'k20_gate', 'k13h', 'k13h_gate', 'k13h_deep', 'k13h_deep_gate', 'k25h' / 'k26h' / 'k27h' /
        # 'k28h' (handed over to the depthwise layer behind) or 'library': what the last forward ran (tests, A/B runs)
        self.last_path = None

    # class-wide switch (tests and A/B runs): 1x1 convolutions on K13 instead of rocBLAS + K10
    use_k13 = True
    # (Cin, Cout, H * W) where K13 measured slower than rocBLAS + K10 (+ x * gate) at the bench shape
    # (EfficientNetV2-S, batch 64, 256 px; DESIGN.md sections 11 and 15): these stay on the library path.  Empty
    # since 1536 -> 256 on 8x8 maps runs K13's 'deep64' tiles
    k13_slower = frozenset()

    def _plain_1x1_call(self, x, c):
        """What K13, K13h and K20 all ask: a plain 1x1 layer (`c`, its conv: a submodule is looked up once per
        question) that emits no mean, a CUDA [B, C, H, W] input, an inference call."""
        return not self.emit_mean and x.is_cuda and x.dim() == 4 and _plain_1x1(c) and _inference_call(c.weight)

    def k13_takes(self, x):
        """Whether forward(x) runs on K13 (conv1x1.hip): a 1x1 stride-1 unpadded ungrouped conv on an f32
        CUDA NCHW-contiguous input, autocast off, no gradient wanted, a shape the C entry accepts."""
        c = self.conv
        return (ConvBiasAct.use_k13 and self._plain_1x1_call(x, c)
                and (c.in_channels, c.out_channels, x.shape[2] * x.shape[3]) not in ConvBiasAct.k13_slower
                and kernels.conv1x1_supported(x, c.weight))

    def k13_accepts(self, x, residual):
        """k13_takes(x), and a skip connection K13's epilogue can add: x's dtype, contiguous, 16-byte aligned."""
        return self.k13_takes(x) and _addable(residual, x)

    # fold_batchnorm(split_gemm=True) sets this on the 1x1, stride-1, unpadded, ungrouped layers of an f32 copy that emit
    # no mean: they run K20 (conv1x1_split.hip, the product on the bf16 matrix cores from split operands) wherever K13
    # would take the input
    split_gemm = False
    # class-wide switch (tests and A/B runs): the armed layers on K13 again
    use_k20 = True
    # (Cin, Cout, H * W) where K20 was not ahead of K13 in every round of tools/conv1x1_ab.py --ab k20 (EfficientNetV2-S
    # batch 64 at 256 px, MobileNetV3 batch 320 at 256 px, EfficientNetV2-L batch 32 at 384 px; DESIGN.md section 23,
    # profiles/r19a_conv1x1_ab_k20_*.jsonl): these keep K13.  All but three are expands (few input channels, many
    # output channels)
    k20_slower = frozenset({(64, 256, 1024), (128, 768, 256), (256, 1536, 64), (256, 1280, 64),
                            (80, 480, 256), (112, 672, 256), (16, 16, 16384), (64, 24, 4096), (72, 24, 4096),
                            (40, 240, 1024), (80, 200, 256), (96, 384, 2304)})
    _ws = None

    def weight_split(self):
        """The conv's weight split for K20 ([3, Cout, Kp] bf16, kernels.pack_conv1x1_split_weight): made on the first
        K20 forward and kept as _derived_weight says."""
        self._ws = _derived_weight(self._ws, self.conv.weight, kernels.pack_conv1x1_split_weight)
        return self._ws[1]

    def _k20_for_k13(self, x):
        """Whether an input that K13 takes goes to K20 instead: an armed layer, the switch on, a shape the C entry
        accepts and that is not listed as slower."""
        if not (self.split_gemm and ConvBiasAct.use_k20):
            return False
        c, hw = self.conv, x.shape[2] * x.shape[3]
        return ((c.in_channels, c.out_channels, hw) not in ConvBiasAct.k20_slower
                and _lib.load().mtr_conv1x1_split_supported(x.shape[0], c.out_channels, c.in_channels, hw) == 0)

    def k20_takes(self, x):
        """Whether forward(x) runs on K20: an armed layer, the switch on, everything k13_takes(x) asks for (so no
        gradient wanted for the weight; like K13 it does not look at x.requires_grad), a shape the C entry accepts and
        that is not listed as slower."""
        return self.split_gemm and self.k13_takes(x) and self._k20_for_k13(x)

    # class-wide switch (tests and A/B runs): 1x1 convolutions of a 16-bit copy on K13h instead of
    # rocBLAS + K10 (+ x * gate)
    use_k13h = True
    # (Cin, Cout, H * W) where K13h measured slower than that library path (unpinned, as the copy runs) in f16 or
    # bf16, both timed as HIP graph replays (EfficientNetV2-S batch 64 at 256 px, EfficientNetV2-L batch 32 at
    # 384 px; DESIGN.md section 12, profiles/r09a_conv1x1_ab_*.jsonl)
    k13h_slower = frozenset({(192, 48, 4096), (256, 64, 1024), (1536, 256, 64), (256, 64, 9216), (768, 192, 576),
                             (1152, 224, 576), (1344, 224, 576), (1344, 384, 144), (2304, 384, 144),
                             (2304, 640, 144), (640, 3840, 144), (3840, 640, 144), (640, 1280, 144)})

    def k13h_takes(self, x):
        """Whether forward(x) runs on K13h (conv1x1_16.hip): a 1x1 stride-1 unpadded ungrouped conv of a 16-bit
        copy (fold_batchnorm(dtype=)) on a CUDA NCHW-contiguous input of the copy's dtype, autocast off, no
        gradient wanted, a shape the C entry accepts."""
        return self._k13h_takes(x, ConvBiasAct.k13h_slower)

    def _k13h_takes(self, x, slower):
        c = self.conv
        return (ConvBiasAct.use_k13h and x.dtype in _16BIT and x.dtype == c.weight.dtype and self._plain_1x1_call(x, c)
                and (c.in_channels, c.out_channels, x.shape[2] * x.shape[3]) not in slower
                and kernels.conv1x1_16_supported(x, c.weight))

    # fold_batchnorm(deep_projects=True) sets this on the deep project convolutions of a 16-bit copy (1x1, stride 1,
    # ungrouped, no activation, Cin >= 768, Cout > 160): they run K13h in `deep_config` wherever K13h takes the input,
    # the shapes of k13h_slower included
    deep_projects = False
    # the K13h configuration of an armed layer (tests and A/B runs set 'auto': the same layers on K13h's old tiles)
    deep_config = 'deepk'
    # (Cin, Cout, H * W) where K13h 'deepk' did not beat the library path an armed layer would otherwise take in every
    # round (EfficientNetV2-L, batch 32, 384 px): these keep today's branch
    k13h_deep_slower = frozenset({(3840, 640, 144)})

    def k13h_deep_takes(self, x):
        """Whether forward(x) runs on K13h in `deep_config`: an armed layer on an input k13h_takes would accept apart
        from the k13h_slower list, unless its shape is in k13h_deep_slower."""
        return self.deep_projects and self._k13h_takes(x, ConvBiasAct.k13h_deep_slower)

    def kernel_for(self, x):
        """The 1x1 kernel that takes `x`, or None.  THE priority order of this class: 'k13h_deep', then 'k13h' (a
        16-bit tensor; K13 and K20 read f32 alone), then 'k20', then 'k13' (an f32 tensor, which K13h refuses); None
        is the library.  A new 1x1 kernel gets its place here."""
        if x.dtype != torch.float32:
            return 'k13h_deep' if self.k13h_deep_takes(x) else 'k13h' if self.k13h_takes(x) else None
        if not self.k13_takes(x):
            return None
        return 'k20' if self._k20_for_k13(x) else 'k13'

    # set by fold_batchnorm(fuse_expand_depthwise=True) on the 1x1 expand of an MBConv block: the stride-1 3x3
    # DepthwiseBiasAct directly behind this layer, which runs both layers as one launch (K25h) -- a reference, as
    # Preproc.hand_to: nothing is registered twice
    hand_to = ()
    # the same reference set by fold_batchnorm(fuse_expand_depthwise_planes=True): that layer runs both as one launch
    # on the planes K25h refuses (K26h).  A field of its own, so the two options never arm one field
    hand_planes_to = ()
    # and by fold_batchnorm(fuse_expand_depthwise_tiles=True): that layer, of stride 1 or 2 and without a mean, runs
    # both as one launch in bands of rows on the large planes the other two refuse (K27h).  Again a field of its own
    hand_tiles_to = ()
    # and by fold_batchnorm(fuse_expand_depthwise5x5=True): the 5x5 DepthwiseBiasAct of stride 1 or 2 behind this
    # layer, which runs both as one launch, with its mean (K28h).  A field of its own once more
    hand_k5_to = ()

    def _handed_kernel(self, x, residual=None, pre=None, defer_epilogue=False):
        """'k25h' / 'k26h' / 'k27h' / 'k28h' where forward(x, ...) hands `x` over to the depthwise layer behind, else
        None.  The three 3x3 kernels' planes are disjoint, and K28h's layers are 5x5."""
        if residual is not None or pre is not None or defer_epilogue:
            return None
        for kernel, cfg in EXPAND_DW_KERNELS.items():
            if any(getattr(dw, cfg['takes'])(x, self) for dw in getattr(self, cfg['field'])):
                return kernel
        return None

    def hands_over(self, x, residual=None, pre=None, defer_epilogue=False):
        """Whether forward(x, ...) leaves `x` untouched to the depthwise layer behind (K25h, K26h, K27h): an armed
        expand, called as the expand of a block is called, and that layer says dw.k25h_takes(x, self) (hand_to),
        dw.k26h_takes(x, self) (hand_planes_to) or dw.k27h_takes(x, self) (hand_tiles_to)."""
        return self._handed_kernel(x, residual, pre, defer_epilogue) is not None

    def path(self, x, residual=None, pre=None, defer_epilogue=False):
        """Which path forward(x, residual, pre=pre, defer_epilogue=defer_epilogue) runs, as last_path will say it:
        'k25h' / 'k26h' / 'k27h' where an armed expand hands `x` over, else the kernel_for(x) if its epilogue can add `residual` ('_gate'
        behind it where the squeeze-excite block in front handed the gate of this very `x` over), 'library' otherwise.
        `x` as it enters the convolution: the first convolution of a 16-bit copy casts before it asks."""
        handed = self._handed_kernel(x, residual, pre, defer_epilogue)
        if handed is not None:
            return handed
        return ConvBiasAct._own_path(self, x, residual, pre, defer_epilogue)

    def _own_path(self, x, residual=None, pre=None, defer_epilogue=False):
        kernel = None if defer_epilogue or not _addable(residual, x) else self.kernel_for(x)
        if kernel is None:
            return 'library'
        held = self._gate if pre is None else None
        return kernel if held is None or held[0] is not x else kernel + '_gate'

    def applies_gate(self, x):
        """To the squeeze-excite block in front: will forward(x) multiply `x` by the gate itself (give_gate), as a
        1x1 kernel stages it?  (A skip that the kernel cannot add sends the call to the library path after all:
        forward multiplies there.)"""
        return self.kernel_for(x) is not None

    def give_gate(self, x, gate):
        """Hands over the squeeze-excite gate [B, C] f32 of `x`: the next forward(x) applies it."""
        self._gate = (x, gate)

    def take_mean_f32(self, x):
        """The [B, C] f32 mean of `x` if `x` is the very tensor this module returned last."""
        held, self._mean = self._mean, None
        if held is not None and held[0] is x:
            return held[1]
        return None

    def take_mean(self, x):
        """The [B, C, 1, 1] mean of `x` (in x's dtype) if `x` is the very tensor this module returned last."""
        m = self.take_mean_f32(x)
        return None if m is None else m.to(x.dtype).view(x.shape[0], x.shape[1], 1, 1)

    def forward(self, x, residual=None, defer_epilogue=False, pre=None):
        """defer_epilogue / pre: between the two layers of an armed FusedMBConv (FusedMBConv._forward_pre) only.
        defer_epilogue=True returns self.conv(x) alone; `pre` is the ConvBiasAct whose conv produced `x` that way:
        its "+ bias, activation" is applied here, inside K13 or K20 where one takes `x`, by K10 in front of the library
        path otherwise.  An armed expand (hand_to, hand_planes_to, hand_tiles_to, hand_k5_to) whose depthwise layer takes
        `x` hands it over and returns it untouched: that layer's forward runs both (K25h, K26h, K27h, K28h)."""
        handed = self._handed_kernel(x, residual, pre, defer_epilogue)
        if handed is not None:
            # decided here, once: the depthwise layer runs this convolution, its bias and its activation itself
            getattr(self, EXPAND_DW_KERNELS[handed]['field'])[0].hand_over(x, self, handed)
            self.last_path = handed
            return x
        return self.forward_here(x, residual, defer_epilogue, pre)

    def forward_here(self, x, residual=None, defer_epilogue=False, pre=None):
        """forward without the hand-over: this layer's own convolution, whatever stands behind it."""
        if defer_epilogue:
            self.last_path = 'library'
            return self.conv(x)
        if pre is None:
            x0, x = x, _to_copy_dtype(x, self.conv.weight)
            if x is not x0 and self._gate is not None and self._gate[0] is x0:
                self._gate = (x, self._gate[1])  # (a gate handed over for the tensor stays with its cast copy)
        # (ConvBiasAct's own order: a subclass has asked for the kernel it puts in front, and of the tensor as it came)
        path = self.last_path = ConvBiasAct._own_path(self, x, residual, pre)
        held, self._gate = self._gate, None
        gate = held[1] if pre is None and held is not None and held[0] is x else None
        if path == 'library':
            if pre is not None:
                x = _finish_bias_act(pre, x, None)
            if gate is not None:  # (the gate was handed over for a 1x1 kernel that cannot add this skip)
                x = x * gate.to(x.dtype).view(x.shape[0], x.shape[1], 1, 1)
            return _library_conv_bias_act(self, x, residual)
        kernel = path if gate is None else path[:-len('_gate')]
        if kernel in ('k13', 'k20'):
            pre_args = {} if pre is None else dict(in_bias=pre.bias, in_act=pre.act_name)
            if kernel == 'k20':
                return kernels.conv1x1_bias_act_split(x, self.weight_split(), self.bias, self.act_name, gate=gate,
                                                      residual=residual, **pre_args)
            return kernels.conv1x1_bias_act(x, self.conv.weight, self.bias, self.act_name, gate=gate,
                                            residual=residual, **pre_args)
        return kernels.conv1x1_bias_act16(x, self.conv.weight, self.bias, self.act_name, gate=gate, residual=residual,
                                          config=ConvBiasAct.deep_config if kernel == 'k13h_deep' else 'auto')


def _library_conv_bias_act(mod, x, residual):
    """The library path of a folded convolution `mod` (ConvBiasAct, Conv3x3BiasAct): mod.conv (MIOpen / rocBLAS),
    then "+ bias, activation (, + residual)" as K10 where it applies, else the torch ops."""
    return _finish_bias_act(mod, mod.conv(x), residual)


def _finish_bias_act(mod, y, residual):
    """The epilogue of the library path on `y` = mod.conv(x)."""
    # K10 moves 16 bytes per lane: planes of a multiple of the vector width (7x7 maps at 224 px,
    # 5x5 at 160 px are not), 16-byte aligned storage; everything else takes the torch ops
    hw_vec_ok = (y.shape[2] * y.shape[3]) % (16 // y.element_size()) == 0
    if y.is_cuda and y.is_contiguous() and hw_vec_ok and y.data_ptr() % 16 == 0 and _addable(residual, y):
        if getattr(mod, 'emit_mean', False) and residual is None:
            y, mean = kernels.bias_act_rowmean_(y, mod.bias, mod.act_name)
            mod._mean = (y, mean)
            return y
        return kernels.bias_act_(y, mod.bias, mod.act_name, residual)
    y = y + mod.bias.view(1, -1, 1, 1).to(y.dtype)
    y = y if mod.act is None else mod.act(y)
    return y if residual is None else residual + y


class Conv3x3BiasAct(nn.Module):
    """A folded dense 3x3 conv + BN (+ activation) of a 16-bit copy (fold_batchnorm(dtype=)): the convolution,
    "+ bias", the activation and the block's skip as ONE HIP launch on the matrix cores (K14h, conv3x3_16.hip)
    instead of a MIOpen convolution followed by K10.  It keeps the folded `conv` (16-bit weight) for every input
    K14h does not take -- channels_last, CPU, autocast, odd maps, a gradient wanted -- which then runs exactly
    what ConvBiasAct runs."""

    # class-wide switch (tests and A/B runs): the library path everywhere
    use_k14h = True
    # (Cin, Cout, stride, H, W) of the input where K14h measured slower than MIOpen (unpinned, as the copy runs) +
    # K10 in f16 or bf16, both timed as HIP graph replays (EfficientNetV2-S and ResNet-18 batch 64 at 256 px,
    # EfficientNetV2-L batch 32 at 384 px; DESIGN.md section 13, profiles/r10a_conv3x3_ab_*.jsonl)
    k14h_slower = frozenset({(64, 256, 2, 96, 96), (64, 64, 1, 64, 64)})

    def __init__(self, conv, bias, act):
        super().__init__()
        self.conv = conv
        self.register_buffer('weight_packed', kernels.pack_conv3x3_weight(conv.weight))  # [Cout, 3, 3, Cin]
        self.register_buffer('bias', bias.detach().float().contiguous())
        self.act = act
        self.act_name = None if act is None else _ACT_NAMES[type(act)]
        self.stride = conv.stride[0]
        self.last_path = None  # 'k14h' or 'library': what the last forward ran (tests, A/B runs)

    @staticmethod
    def applies_to(conv):
        return _dense_3x3(conv, strides=((1, 1), (2, 2))) and conv.in_channels % 8 == 0

    def k14h_takes(self, x):
        """Whether forward(x) runs on K14h: a CUDA NCHW-contiguous input of the copy's dtype, autocast off, no
        gradient wanted, a shape the C entry accepts and that is not listed as slower."""
        c = self.conv
        if not (Conv3x3BiasAct.use_k14h and x.is_cuda and x.dim() == 4 and x.dtype == c.weight.dtype
                and x.dtype in _16BIT and c.bias is None and _inference_call(c.weight)):
            return False
        if (c.in_channels, c.out_channels, self.stride, x.shape[2], x.shape[3]) in Conv3x3BiasAct.k14h_slower:
            return False
        return kernels.conv3x3_16_supported(x, self.weight_packed, self.stride)

    def path(self, x, residual=None):
        """Which path forward(x, residual) runs, as last_path will say it: 'k14h', then 'library'.  `x` as it enters
        the convolution (the first convolution of a 16-bit copy casts before it asks)."""
        return 'k14h' if self.k14h_takes(x) and _addable(residual, x) else 'library'

    def forward(self, x, residual=None):
        x = _to_copy_dtype(x, self.conv.weight)
        self.last_path = self.path(x, residual)
        if self.last_path == 'k14h':
            return kernels.conv3x3_bias_act16(x, self.weight_packed, self.bias, self.act_name, self.stride,
                                              residual=residual)
        return _library_conv_bias_act(self, x, residual)


class StemConvBiasAct(ConvBiasAct):
    """The folded stem -- a dense 3x3, stride-2, padding-1, Cin = 3 conv + BN + activation -- of a copy made with
    fold_batchnorm(fuse_stem=True): Preproc, the convolution, "+ bias" and the activation as ONE HIP launch (K17,
    stem_conv.hip) instead of an elementwise pass, a MIOpen convolution and K10.  K17 reads contiguous and
    channels_last (interleaved) crops in place and writes an NCHW-contiguous activation.  Same parameters and
    state_dict keys as the ConvBiasAct it replaces, which it also is for every input K17 does not take -- CPU,
    autocast, a gradient wanted, odd shapes, other strides: those run exactly what ConvBiasAct runs."""

    # class-wide switch (tests and A/B runs): the library path everywhere
    use_k17 = True
    # (Cout, H, W) of the input where K17 measured slower than Preproc + MIOpen + K10.  Empty
    # because no shape has been timed yet, not because every shape is ahead
    k17_slower = frozenset()

    def __init__(self, conv, bias, act):
        super().__init__(conv, bias, act)  # (last_path: 'k17' or 'library')
        self._handed = None

    @staticmethod
    def applies_to(conv):
        return _dense_3x3(conv, strides=((2, 2),)) and conv.in_channels == 3

    def k17_takes(self, x):
        """Whether forward(x) runs on K17: a CUDA input, contiguous or channels_last, of the copy's dtype (or f32 in
        front of a 16-bit copy), autocast off, no gradient wanted, a shape the C entry accepts and that is not listed
        as slower."""
        c = self.conv
        if not (StemConvBiasAct.use_k17 and x.is_cuda and x.dim() == 4 and c.bias is None and not self.emit_mean
                and _inference_call(c.weight, x=x)):
            return False
        if (c.out_channels, x.shape[2], x.shape[3]) in StemConvBiasAct.k17_slower:
            return False
        return kernels.stem_conv_supported(x, c.weight)

    def path(self, x, residual=None):
        """'k17' in front of ConvBiasAct's order (which, for a 3x3 layer, says 'library')."""
        return 'k17' if residual is None and self.k17_takes(x) else super().path(x, residual)

    def hand_over(self, x):
        """From the Preproc in front: `x` comes WITHOUT x * 2 - 1 applied; the next forward(x) applies it."""
        self._handed = x

    def forward(self, x, residual=None):
        held, self._handed = self._handed, None
        raw = held is not None and held is x  # Preproc left x * 2 - 1 to this module
        if self.path(x, residual) == 'k17':
            self.last_path = 'k17'
            return kernels.stem_conv_bias_act(x, self.conv.weight, self.bias, self.act_name, preproc=raw)
        if raw:  # (Preproc asked k17_takes(x) before it handed x over; whatever changed since: never un-preprocessed)
            x = x * 2 - 1
        return super().forward(x, residual)


class Dense3x3BiasAct(ConvBiasAct):
    """What the three classes below share: a folded dense 3x3, padding-1 conv + BN (+ activation) of an f32 copy whose
    convolution, "+ bias", activation and skip run as ONE HIP launch on a kernel of DENSE3X3_KERNELS instead of a MIOpen
    convolution followed by K10.  Same parameters and state_dict keys as the ConvBiasAct it replaces (the packed weight
    is derived state, cached per kernel, weight storage and version), which it also is for every input no armed kernel
    takes -- CPU, channels_last, autocast, a gradient wanted, the shapes the entry refuses or the class lists as
    slower: those run exactly what ConvBiasAct runs.  A subclass names its `kernel`, whose row says the rest."""

    kernel = None  # the key of DENSE3X3_KERNELS whose row names this class

    # (last_path: an armed kernel or what ConvBiasAct says)

    @staticmethod
    def classes():
        """The classes the table names, in its order."""
        return tuple(globals()[row['cls']] for row in DENSE3X3_KERNELS.values())

    @classmethod
    def applies_to(cls, conv):
        row = DENSE3X3_KERNELS[cls.kernel]
        return _dense_3x3(conv, strides=((row['stride'],) * 2,)) and conv.in_channels % row['cin_multiple'] == 0

    def armed(self):
        """The kernels this layer may run, in the table's order."""
        return (self.kernel,)

    def packed_weight(self, kernel):
        """The conv's weight as `kernel` reads it (its row's packer in kernels): made on the first forward that runs
        the kernel and kept in the row's slot as _derived_weight says."""
        row = DENSE3X3_KERNELS[kernel]
        held = _derived_weight(getattr(self, row['slot'], None), self.conv.weight, getattr(kernels, row['pack']))
        setattr(self, row['slot'], held)
        return held[1]

    def takes(self, kernel, x):
        """Whether forward(x) may run on `kernel`: the layer is armed for it and its class-wide switch is on, a CUDA
        NCHW-contiguous f32 input, autocast off, no gradient wanted, a shape the C entry accepts and that is not listed
        as slower."""
        row = DENSE3X3_KERNELS[kernel]
        cls, c = globals()[row['cls']], self.conv
        if not (kernel in self.armed() and getattr(cls, row['switch']) and not self.emit_mean and x.is_cuda
                and x.dim() == 4 and x.dtype == torch.float32 and c.weight.dtype == torch.float32 and c.weight.is_cuda
                and c.bias is None and x.is_contiguous() and x.data_ptr() % 16 == 0
                and _inference_call(c.weight, x=x)):
            return False
        B, K, H, W = x.shape
        if K != c.in_channels or (K, c.out_channels, H, W) in getattr(cls, row['slower']):
            return False
        return getattr(_lib.load(), row['query'])(B, K, c.out_channels, H, W) > 0

    def path(self, x, residual=None, pre=None, defer_epilogue=False):
        """The first armed kernel that takes `x` and whose epilogue can add `residual`, in front of ConvBiasAct's order
        (which, for a 3x3 layer, says 'library')."""
        if not defer_epilogue and pre is None:
            for kernel in self.armed():
                s = DENSE3X3_KERNELS[kernel]['stride']
                if self.takes(kernel, x) and _addable(
                        residual, x, shape=(x.shape[0], self.conv.out_channels, x.shape[2] // s, x.shape[3] // s)):
                    return kernel
        return ConvBiasAct.path(self, x, residual, pre, defer_epilogue)

    def forward(self, x, residual=None, defer_epilogue=False, pre=None):
        kernel = self.path(x, residual, pre, defer_epilogue)
        if kernel in DENSE3X3_KERNELS:
            self.last_path = kernel
            return getattr(kernels, DENSE3X3_KERNELS[kernel]['fn'])(x, self.packed_weight(kernel), self.bias,
                                                                    self.act_name, residual=residual)
        return ConvBiasAct.forward(self, x, residual=residual, defer_epilogue=defer_epilogue, pre=pre)


class WinogradConv3x3BiasAct(Dense3x3BiasAct):
    """A stride-1 layer with Cin % 4 == 0 of a copy made with fold_batchnorm(winograd3x3=True): Winograd F(2x2, 3x3) on
    the f32 MFMA (K19, conv3x3_winograd.hip; the weight as [16, Cout, Cin], last_path 'k19')."""

    kernel = 'k19'
    # class-wide switch (tests and A/B runs): the library path everywhere
    use_k19 = True
    # (Cin, Cout, H, W) of the input where K19 (for the expand of a FusedMBConv: K19 + the plain K13 project) was not
    # ahead of the default copy's path in every round of tools/conv3x3_ab.py --dtype f32 (EfficientNetV2-S and ResNet-18
    # batch 64 at 256 px, EfficientNetV2-L batch 32 at 384 px; DESIGN.md section 22, profiles/r18a_conv3x3_ab_winograd_*.jsonl)
    k19_slower = frozenset({(512, 512, 8, 8)})

    def weight_u(self):
        return self.packed_weight('k19')

    def k19_takes(self, x):
        return self.takes('k19', x)


class SplitConv3x3BiasAct(WinogradConv3x3BiasAct):
    """A stride-1 layer with Cin % 8 == 0 of a copy made with fold_batchnorm(split3x3=True): the convolution on the bf16
    matrix cores from operands split into three bf16 pieces each, K20's arithmetic (K21, conv3x3_split.hip; the weight
    as [3, Cout, 3, 3, Cp] bf16, last_path 'k21').  It derives from WinogradConv3x3BiasAct so that one layer can hold
    both options: `winograd` says whether winograd3x3 was on too.  Where K21 refuses the input or lists the shape, the
    layer runs K19 if `winograd` and K19 takes it, and exactly what ConvBiasAct runs everywhere else."""

    kernel = 'k21'
    # class-wide switch (tests and A/B runs): what the copy without split3x3 runs, everywhere
    use_k21 = True
    # (Cin, Cout, H, W) of the input where K21 (for the expand of a FusedMBConv: K21 + the plain K13 project) was not
    # ahead of the default copy's path in every round of tools/conv3x3_ab.py --dtype f32 (EfficientNetV2-S and ResNet-18
    # batch 64 at 256 px, EfficientNetV2-L batch 32 at 384 px; DESIGN.md section 34,
    # profiles/r25a_conv3x3_ab_k21_*.jsonl): the small maps of ResNet-18 -- one tile per image on 16x16 maps (at batch
    # 64 fewer workgroups than CUs), a quarter of a tile on 8x8 maps
    k21_slower = frozenset({(256, 256, 16, 16), (512, 512, 8, 8)})

    def __init__(self, conv, bias, act, winograd=False):
        super().__init__(conv, bias, act)
        self.winograd = bool(winograd)

    def armed(self):
        return ('k21', 'k19') if self.winograd else ('k21',)

    def weight_split3(self):
        return self.packed_weight('k21')

    def k21_takes(self, x):
        return self.takes('k21', x)


class StridedConv3x3BiasAct(Dense3x3BiasAct):
    """A stride-2 layer with Cin % 4 == 0 of a copy made with fold_batchnorm(strided3x3=True): an implicit GEMM on the
    f32 MFMA (K22, conv3x3_strided.hip; the weight as [Cin / 4, Cout, 3, 3, 4], last_path 'k22')."""

    kernel = 'k22'
    # class-wide switch (tests and A/B runs): the library path everywhere
    use_k22 = True
    # (Cin, Cout, H, W) of the input where K22 (for the expand of a FusedMBConv: K22 + the plain K13 project) was not
    # ahead of the default copy's path in every round of tools/conv3x3_ab.py --dtype f32
    k22_slower = frozenset()

    def weight_s(self):
        return self.packed_weight('k22')

    def k22_takes(self, x):
        return self.takes('k22', x)


class DepthwiseBiasAct(nn.Module):
    """A folded depthwise 3x3 (K11) or 5x5 (K15) conv + BN + activation as ONE HIP pass over the plane: the
    convolution, "+ bias", the activation and -- in front of a squeeze-excite block -- the
    per-channel mean, instead of PyTorch's depthwise kernel followed by K10.  Other tensors (CPU,
    non-contiguous, widths that are not a multiple of 4; for 5x5 also padded planes above 112 x 112 and the shapes
    in k15_slower) take the torch ops at the layer's own kernel size and padding."""

    # kernel sizes fold_batchnorm hands to this class (read at fold time: tests and A/B runs set (3,) to get
    # the 5x5 layers as ConvBiasAct around DepthwiseConv2d, the module tree from before K15)
    kernel_sizes = (3, 5)
    # (C, H, W, stride) of the input where K15 measured slower than PyTorch's depthwise kernel + K10: these
    # run the torch ops
    k15_slower = frozenset()
    # K18 (fold_batchnorm(block_depthwise=True)): the class-wide switch, and the (C, H, W) of the input where K18
    # measured slower than K11: these stay on K11
    use_k18 = True
    k18_slower = frozenset()

    def __init__(self, conv, bias, act):
        super().__init__()
        self.weight = nn.Parameter(conv.weight.detach().float().contiguous(), requires_grad=False)
        self.register_buffer('bias', bias.detach().float().contiguous())
        self.k = conv.kernel_size[0]
        self.stride, self.pad = conv.stride[0], conv.padding[0]
        # (left, right, top, bottom) of a ZeroPad2d that stood in front of the layer and was folded
        # in by fold_batchnorm (the TF-'SAME' padding of the stride-2 layers); None: self.pad all round
        self.pads = None
        self.act = act
        self.act_name = None if act is None else _ACT_NAMES[type(act)]
        self.emit_mean = False
        self._mean = None
        self.last_path = None  # 'k11', 'k15', 'k18', 'k25h', 'k26h', 'k27h', 'k28h' or 'library': what the last forward ran (tests, A/B runs)
        # fold_batchnorm(block_depthwise=True) sets this on the k = 3, stride-1, padding-1 layers: they run K18 on
        # the planes it takes and K11's block kernel refuses -- the bits of K11's generic kernel, which those planes
        # run on otherwise
        self.block_depthwise = False

    @classmethod
    def applies_to(cls, conv):
        k = conv.kernel_size[0] if isinstance(conv, nn.Conv2d) else None
        return (isinstance(conv, nn.Conv2d) and conv.groups == conv.in_channels == conv.out_channels
                and conv.groups > 1 and k in cls.kernel_sizes and conv.kernel_size == (k, k)
                and conv.dilation == (1, 1) and conv.stride in ((1, 1), (2, 2))
                and conv.padding in ((0, 0), (k // 2, k // 2)) and conv.padding_mode == 'zeros')

    take_mean = ConvBiasAct.take_mean
    take_mean_f32 = ConvBiasAct.take_mean_f32

    def _k18_takes(self, x):
        """An armed layer's input (cuda, contiguous, f32 / f16 / bf16) goes to K18 instead of K11."""
        B, C, H, W = x.shape
        return (DepthwiseBiasAct.use_k18 and _autocast_off()
                and self.stride == 1 and self.pads is None
                and kernels.depthwise3x3_blocks_supported(x.dtype, H, W, self.stride, self.pad, x.data_ptr())
                and not kernels.k11_takes_block_kernel(H, W) and 0 < B * C < 2 ** 24
                and (C, H, W) not in DepthwiseBiasAct.k18_slower)

    # K25h (fold_batchnorm(fuse_expand_depthwise=True)): the class-wide switch, and the (Cin, Cmid, H, W) of the
    # expand's input where K25h was not ahead of the chain K13h + K11 in every round of tools/expand_dw_ab.py: these
    # keep the chain (EfficientNetV2-S batch 64 and MobileNetV3 batch 320 at 256 px, f16 and bf16, the same five in
    # both; DESIGN.md section 30, profiles/r21a_expand_dw_ab.jsonl).  EfficientNetV2-L and other resolutions have not
    # been timed
    use_k25h = True
    k25h_slower = frozenset({(128, 768, 16, 16), (160, 960, 16, 16), (80, 200, 16, 16), (80, 480, 16, 16),
                             (112, 672, 16, 16)})
    _handed = None

    def _expand_dw_candidate(self, x, expand, strides, switch, k=3, pad=1):
        """What k25h_takes, k26h_takes, k27h_takes and k28h_takes ask first: the class-wide `switch` is on, this is a
        `k` x `k` padding-`pad` layer (3 and 1; K28h: 5 and 2) of a stride in `strides` without a folded ZeroPad2d, an
        inference call on both weights, a CUDA NCHW-contiguous input of the copy's dtype that `expand` would run on
        K13h with no gate held."""
        c = expand.conv
        if not (getattr(DepthwiseBiasAct, switch) and self.k == k and self.stride in strides and self.pad == pad
                and self.pads is None and x.is_cuda and x.dim() == 4 and x.is_contiguous() and x.dtype in _16BIT
                and x.dtype == c.weight.dtype and _inference_call(c.weight, self.weight)):
            return False
        held = expand._gate
        return not (held is not None and held[0] is x) and expand.kernel_for(x) == 'k13h'

    def k25h_takes(self, x, expand):
        """Whether this layer runs `expand` (the armed 1x1 ConvBiasAct in front) and itself on `x`, the expand's input,
        as one launch (K25h, expand_dw16.hip): a 3x3 stride-1 padding-1 layer without a folded ZeroPad2d, an inference
        call on both weights, a CUDA NCHW-contiguous input of the copy's dtype that the expand would run on K13h with
        no gate held, a plane K11 runs on its block kernel, a shape the C entry accepts and that is not listed as
        slower.  Everything else runs the chain: today's branch, today's bits."""
        if not self._expand_dw_candidate(x, expand, (1,), 'use_k25h', 3, 1):
            return False
        c, (B, K, H, W) = expand.conv, x.shape
        return (kernels.k11_takes_block_kernel(H, W)
                and (K, c.out_channels, H, W) not in DepthwiseBiasAct.k25h_slower
                and kernels.expand_depthwise16_supported(x, c.weight))

    # K26h (fold_batchnorm(fuse_expand_depthwise_planes=True)): the class-wide switch, and the (Cin, Cmid, H, W) of the
    # expand's input where K26h was not ahead of the chain K13h + K11 in every round of tools/expand_dw_ab.py --kernel
    # k26h: EVERY class timed so far (EfficientNetV2-L batch 32 and -S batch 64 at 384 px, f16 and bf16, the same eight
    # in both, 0.58 - 0.96x; DESIGN.md section 31, profiles/r22a_expand_dw_ab_k26h.jsonl).  As shipped the armed pairs
    # of those two networks therefore keep the chain at 384 px; MobileNetV3 and other planes have not been timed
    use_k26h = True
    k26h_slower = frozenset({(192, 768, 24, 24), (192, 1152, 24, 24), (224, 1344, 24, 24), (384, 2304, 12, 12),
                             (128, 512, 24, 24), (128, 768, 24, 24), (160, 960, 24, 24), (256, 1536, 12, 12)})

    def k26h_takes(self, x, expand):
        """k25h_takes for K26h (expand_dw16_planes.hip): the same conditions, but the plane is one K11 does NOT run on
        its block kernel -- 24x24, 12x12 -- and the C entry of K26h accepts the shape."""
        if not self._expand_dw_candidate(x, expand, (1,), 'use_k26h', 3, 1):
            return False
        c, (B, K, H, W) = expand.conv, x.shape
        return (not kernels.k11_takes_block_kernel(H, W)
                and (K, c.out_channels, H, W) not in DepthwiseBiasAct.k26h_slower
                and kernels.expand_depthwise16_planes_supported(x, c.weight))

    # K27h (fold_batchnorm(fuse_expand_depthwise_tiles=True)): the class-wide switch, and the (Cin, Cmid, H, W, stride)
    # of the expand's input where K27h was not ahead of the chain K13h + K11 in every round of tools/expand_dw_ab.py
    # --kernel k27h: MobileNetV3's 40 -> 240 at 32x32, stride 2 (0.69 - 0.70x; batch 320 at 256 px, f16 and bf16).  Its
    # 24 -> 72 at 64x64 (1.80 - 1.82x) and 16 -> 64 at 128x128, stride 2 (1.16 - 1.18x) are ahead in every round
    # (profiles/r23a_expand_dw_ab_k27h.jsonl).  Other networks, planes and batch sizes have not
    # been timed
    use_k27h = True
    k27h_slower = frozenset({(40, 240, 32, 32, 2)})

    def k27h_takes(self, x, expand):
        """k26h_takes for K27h (expand_dw16_tiles.hip): the same conditions, but this layer emits no mean, has stride 1
        or 2, and the plane is one of stride 2, or a stride-1 plane that is neither a block-kernel plane (K25h's, or the
        chain's with other bits) nor one K26h's entry accepts -- so the three kernels never compete for a plane -- and
        the C entry of K27h accepts the shape."""
        if self.emit_mean or not self._expand_dw_candidate(x, expand, (1, 2), 'use_k27h', 3, 1):
            return False
        c, (B, K, H, W) = expand.conv, x.shape
        if self.stride == 1 and (kernels.k11_takes_block_kernel(H, W)
                                 or kernels.expand_depthwise16_planes_supported(x, c.weight)):
            return False
        return ((K, c.out_channels, H, W, self.stride) not in DepthwiseBiasAct.k27h_slower
                and kernels.expand_depthwise16_tiles_supported(x, c.weight, self.stride))

    # K28h (fold_batchnorm(fuse_expand_depthwise5x5=True)): the class-wide switch, and the (Cin, Cmid, H, W, stride) of
    # the expand's input where K28h was not ahead of the chain K13h + K15 in every round of tools/expand_dw_ab.py
    # --kernel k28h: EVERY class timed so far (MobileNetV3 batch 320 at 256 px, f16 and bf16, the same three in both,
    # 0.52 - 0.61x; DESIGN.md section 36, profiles/r26a_expand_dw_ab_k28h.jsonl).  As shipped the armed pairs of that
    # network therefore keep the chain at 256 px; other resolutions, batch sizes and networks have not been timed
    use_k28h = True
    k28h_slower = frozenset({(40, 120, 32, 32, 1), (112, 672, 16, 16, 2), (160, 960, 8, 8, 1)})

    def k28h_takes(self, x, expand):
        """k25h_takes for K28h (expand_dw16_k5.hip): this is a 5x5 padding-2 layer of stride 1 or 2 without a folded
        ZeroPad2d, with or without a mean, that would run K15 on the expanded tensor (what path() says of it); the
        shape is not listed as slower and the C entry of K28h accepts it."""
        if not self._expand_dw_candidate(x, expand, (1, 2), 'use_k28h', 5, 2):
            return False
        c, (B, K, H, W) = expand.conv, x.shape
        return ((c.out_channels, H, W, self.stride) not in DepthwiseBiasAct.k15_slower
                and kernels.depthwise5x5_supported(H, W, self.pad)
                and (K, c.out_channels, H, W, self.stride) not in DepthwiseBiasAct.k28h_slower
                and kernels.expand_depthwise16_k5_supported(x, c.weight, self.stride))

    def hand_over(self, x, expand, kernel='k25h'):
        """From the armed expand in front: `x` comes WITHOUT that convolution applied; the next forward(x) runs it, on
        `kernel` ('k25h' / 'k26h' / 'k27h' / 'k28h') where this layer still takes it."""
        self._handed = (x, expand, kernel)

    def path(self, x):
        """Which path forward(x) runs on an input that was not handed over, as last_path will say it: 'k18' (an armed
        3x3 layer), then 'k11' (3x3) or 'k15' (5x5), then 'library' (the torch ops).  ('k25h' / 'k26h' / 'k27h' / 'k28h':
        forward, on the input an armed expand handed over.)"""
        pl, pr = (self.pad, self.pad) if self.pads is None else self.pads[:2]
        ow = (x.shape[3] + pl + pr - self.k) // self.stride + 1
        if not (x.is_cuda and x.is_contiguous() and ow % 4 == 0 and x.dtype in _FLOATS):
            return 'library'
        if self.k == 3:
            return 'k18' if self.block_depthwise and self._k18_takes(x) else 'k11'
        if (x.shape[1], x.shape[2], x.shape[3], self.stride) not in DepthwiseBiasAct.k15_slower and \
                kernels.depthwise5x5_supported(x.shape[2], x.shape[3], self.pad if self.pads is None else self.pads):
            return 'k15'
        return 'library'

    def forward(self, x):
        held, self._handed = self._handed, None
        if held is not None and held[0] is x:  # the expand in front left its convolution to this module
            expand, kernel = held[1], held[2]
            cfg = EXPAND_DW_KERNELS[kernel]
            if getattr(self, cfg['takes'])(x, expand):
                self.last_path = kernel
                # (what the row says: the stride as an argument, the mean where the kernel has one -- a layer of a
                # kernel without a mean emits none)
                extra = dict(stride=self.stride) if cfg['strided'] else {}
                if cfg['mean']:
                    extra['want_mean'] = self.emit_mean
                out = getattr(kernels, cfg['fn'])(x, expand.conv.weight, expand.bias, expand.act_name, self.weight,
                                                  self.bias, self.act_name, **extra)
                if not self.emit_mean:
                    return out
                self._mean = out
                return out[0]
            # (the expand asked k25h_takes / k26h_takes / k27h_takes / k28h_takes before it handed x over; whatever
            # changed since: never un-expanded)
            x = expand.forward_here(x)
        path = self.last_path = self.path(x)
        if path != 'library':
            if path == 'k18':
                fn, geometry = kernels.depthwise3x3_blocks_bias_act, ()
            else:
                fn = kernels.depthwise3x3_bias_act if path == 'k11' else kernels.depthwise5x5_bias_act
                geometry = (self.stride, self.pad if self.pads is None else self.pads)
            if not self.emit_mean:
                return fn(x, self.weight, self.bias, self.act_name, *geometry)
            y, mean = fn(x, self.weight, self.bias, self.act_name, *geometry, want_mean=True)
            self._mean = (y, mean)
            return y
        if self.pads is not None:
            x = F.pad(x, self.pads)
        y = F.conv2d(x, self.weight.to(x.dtype), self.bias.to(x.dtype), self.stride,
                     self.pad if self.pads is None else 0, groups=self.weight.shape[0])
        return y if self.act is None else self.act(y)


def _block_plus_skip(block, x):
    """x + block(x) of an (Fused)MBConv; when the block ends in a folded convolution (ConvBiasAct,
    Conv3x3BiasAct) the skip connection rides on its epilogue instead of being a kernel of its own."""
    last = block[-1]
    tail = last[0] if isinstance(last, ConvBNAct) else None
    if isinstance(tail, (ConvBiasAct, Conv3x3BiasAct)):
        y = x
        for m in list(block)[:-1]:
            y = m(y)
        for m in list(last)[1:]:
            assert isinstance(m, nn.Identity)
        return tail(y, residual=x)
    return x + block(x)


# ---- fold_batchnorm: the steps, in the order fold_batchnorm calls them

def _adjacent_children(net):
    """(sequential, name of a, a, b) for every two adjacent children a, b of the Sequentials of `net` that are no
    ConvBNAct: where one layer is wired to the next."""
    for seq in net.modules():
        if isinstance(seq, nn.Sequential) and not isinstance(seq, ConvBNAct):
            names = list(seq._modules)
            for a, b in zip(names, names[1:]):
                yield seq, a, seq._modules[a], seq._modules[b]


def _only_layer(blk):
    """The folded layer of a ConvBNAct whose other children are folded away (Identity), else None."""
    if isinstance(blk, ConvBNAct) and all(isinstance(m, nn.Identity) for m in list(blk)[1:]):
        return blk[0]
    return None


def _expand_and_project(m, expand_classes):
    """(expand, project) of a FusedMBConv whose block is exactly a dense 3x3 layer of one of `expand_classes` and a
    plain 1x1 ConvBiasAct project without activation, neither emitting a mean; None for every other module."""
    if not isinstance(m, FusedMBConv) or list(m.block._modules) != ['0', '1']:
        return None
    expand, project = _only_layer(m.block._modules['0']), _only_layer(m.block._modules['1'])
    if type(expand) in expand_classes and type(project) is ConvBiasAct \
            and expand.conv.kernel_size == (3, 3) and expand.conv.groups == 1 \
            and not getattr(expand, 'emit_mean', False) and project.act is None and not project.emit_mean \
            and _plain_1x1(project.conv) and project.conv.in_channels == expand.conv.out_channels:
        return expand, project
    return None


def _replace_conv_bias_act(folded, cls, first_only=False):
    """Makes every ConvBiasAct (the first one alone: first_only) that emits no mean and whose conv cls.applies_to a
    `cls` around the same conv, bias and activation: same parameters, same state_dict keys.  -> the ConvBNAct blocks."""
    done = []
    for m in folded.modules():
        if isinstance(m, ConvBNAct) and type(m[0]) is ConvBiasAct and not m[0].emit_mean and cls.applies_to(m[0].conv):
            m[0] = cls(m[0].conv, m[0].bias, m[0].act)
            done.append(m)
            if first_only:
                break
    return done


def _fold_convs(folded, fused_epilogue):
    """Every ConvBNAct: the batch norm folded into the convolution (w' = w * gamma / sqrt(var + eps), b' = beta -
    mean * gamma / sqrt(var + eps)); with fused_epilogue the conv becomes a ConvBiasAct (K10), or a DepthwiseBiasAct
    (K11, K15) where that class applies."""
    from torch.nn.utils.fusion import fuse_conv_bn_eval
    for m in folded.modules():
        if isinstance(m, ConvBNAct) and isinstance(m[1], nn.BatchNorm2d):
            conv = fuse_conv_bn_eval(m[0], m[1])
            act = m[2] if len(m) > 2 else None
            if fused_epilogue and (act is None or type(act) in _ACT_NAMES):
                bias, conv.bias = conv.bias, None
                m[0] = (DepthwiseBiasAct if DepthwiseBiasAct.applies_to(conv) else ConvBiasAct)(
                    conv, bias, act)
                if act is not None:
                    m[2] = nn.Identity()
            else:
                m[0] = conv
            m[1] = nn.Identity()
    if any(isinstance(m, nn.BatchNorm2d) for m in folded.modules()):
        raise ValueError('a BatchNorm2d outside a ConvBNAct block cannot be folded here')


def _fold_paddings(folded):
    """ZeroPad2d -> depthwise 3x3 / 5x5: the padding becomes an argument of K11 / K15."""
    for seq, n_pad, pad, blk in _adjacent_children(folded):
        if isinstance(pad, nn.ZeroPad2d) and isinstance(blk, ConvBNAct) and \
                isinstance(blk[0], DepthwiseBiasAct) and blk[0].pad == 0:
            l, r, t, b = (int(p) for p in pad.padding)
            lo, hi = blk[0].k // 2, blk[0].k // 2 + 1  # what the C entries take: 1 / 2 (3x3), 2 / 3 (5x5)
            if 0 <= l <= lo and 0 <= t <= lo and 0 <= r <= hi and 0 <= b <= hi:
                blk[0].pads = (l, r, t, b)
                seq._modules[n_pad] = nn.Identity()


def _wire_squeeze_excite(folded):
    """conv -> squeeze-excite: the epilogue pass in front also emits the channel means (mean_from, emit_mean).
    squeeze-excite -> project conv: the gate multiplies the project conv's input inside its 1x1 kernel (gate_to)."""
    for _, _, prev, nxt in _adjacent_children(folded):
        if isinstance(nxt, SqueezeExcite) and isinstance(_only_layer(prev), (ConvBiasAct, DepthwiseBiasAct)):
            prev[0].emit_mean = True
            nxt.mean_from = (prev[0],)
        if isinstance(prev, SqueezeExcite) and isinstance(nxt, ConvBNAct) and isinstance(nxt[0], ConvBiasAct):
            prev.gate_to = (nxt[0],)


def _replace_dense3x3(folded, options):
    """split3x3, winograd3x3, strided3x3: every dense 3x3, padding-1, ungrouped ConvBiasAct that emits no mean, of the
    stride and with the Cin multiple of the option's row of DENSE3X3_KERNELS, becomes that row's class, in the table's
    order -- so the split layers are taken when winograd3x3 looks for its own, and `winograd` on them says whether it
    was on as well.  Stride 1: 8 layers of EfficientNetV2-S, 16 of -L, 13 of ResNet-18, none of MobileNetV3 (every
    such layer has Cin % 8 == 0).  Stride 2: 2 of EfficientNetV2-S, 2 of -L, 3 of ResNet-18, none of MobileNetV3 (the
    stems have Cin = 3 and stay K17's).  Such a layer runs the convolution, "+ bias", the activation and the block's
    skip in one launch (.last_path 'k21', 'k19' or 'k22') where an armed kernel takes the input and the shape is not
    in its class's list of slower shapes -- a split layer K21, else K19 where winograd3x3 is on too -- and exactly
    what ConvBiasAct runs everywhere else.  An armed FusedMBConv expand block runs that kernel with its own epilogue
    and then the project as a plain K13 call -- a plain K20 call with split_gemm=True -- (block .last_path the same).
    K19 and K22 differ from the default copy's results by rounding (other summation orders); K21 is f32-grade against
    fp64 but not the library's bits."""
    for row in DENSE3X3_KERNELS.values():
        if options[row['option']]:
            for blk in _replace_conv_bias_act(folded, globals()[row['cls']]):
                if isinstance(blk[0], SplitConv3x3BiasAct):
                    blk[0].winograd = bool(options['winograd3x3'])


def _arm_pre_pairs(folded):
    """An f32 copy: every FusedMBConv whose block is exactly a dense 3x3 ConvBiasAct (or the class of
    Dense3x3BiasAct.classes() that replaced it) and a 1x1 ConvBiasAct project without activation is armed: the 3x3
    layer's K10 pass is left out
    and applied by the project's K13 launch as it stages its input (FusedMBConv.pre_pair, .last_path 'k13_pre'), with
    the bits of the chain, which runs wherever K13 does not take the tensor.  Same module tree, same state_dict."""
    for m in folded.modules():
        pair = _expand_and_project(m, (ConvBiasAct,) + Dense3x3BiasAct.classes())
        if pair:
            m.pre_pair = pair


def _cast_16bit(folded, dtype):
    """The 16-bit copy: every convolution weight that runs as a GEMM or MIOpen convolution (1x1, dense 3x3, stem,
    ResNet convs) is cast to `dtype` once, not by autocast on every forward.  The folded biases, the depthwise layers
    (K11, K15) and the squeeze-excite blocks (K12) keep f32 parameters.  The copy computes in `dtype` (its input is
    cast at the first convolution; run it with autocast off), its 1x1 stride-1 convolutions run on K13h, and its dense
    3x3 convolutions (stride 1 or 2, padding 1, Cin a multiple of 8) become Conv3x3BiasAct: K14h, on the weight
    repacked once."""
    for m in folded.modules():
        if isinstance(m, ConvBiasAct):
            m.conv.to(dtype)
    _replace_conv_bias_act(folded, Conv3x3BiasAct)
    folded.inference_dtype = dtype


def _arm_fused_pairs(folded):
    """fuse_blocks: every FusedMBConv whose block is exactly a Conv3x3BiasAct expand and a ConvBiasAct project without
    activation runs as ONE launch (K16h) where that kernel takes the input, with the bits of the two-kernel chain, and
    the chain everywhere else (block .last_path 'k16h' / 'chain'; an unarmed block reports None)."""
    for m in folded.modules():
        pair = _expand_and_project(m, (Conv3x3BiasAct,))
        if pair:
            m.fused_pair = pair


def _arm_block_depthwise(folded):
    """block_depthwise: every 3x3, stride-1, padding-1 DepthwiseBiasAct without a folded ZeroPad2d runs K18, the
    register-block kernel, on the planes that kernel takes and K11's own block kernel refuses (24x24 and 12x12 of
    EfficientNetV2 at 384 px, 128x128 and 64x64 of MobileNetV3 at 256 px), and K11 everywhere else.  K18 returns the
    bits of K11's generic kernel for the output and the mean, so the armed copy's features are torch.equal to the
    default copy's."""
    for m in folded.modules():
        if isinstance(m, DepthwiseBiasAct) and m.k == 3 and m.stride == 1 and m.pad == 1 and m.pads is None:
            m.block_depthwise = True


def _arm_deep_projects(folded):
    """deep_projects: every plain 1x1 ConvBiasAct without activation that has Cin >= 768 and Cout > 160 -- the deep
    project convolutions of the MBConv tails: 15 layers of EfficientNetV2-S, 60 of EfficientNetV2-L, none of
    MobileNetV3 or ResNet.  An armed layer runs K13h in its deep-K configuration (ConvBiasAct.deep_config, .last_path
    'k13h_deep' / 'k13h_deep_gate') with the squeeze-excite gate and the skip folded in, wherever K13h takes the input
    -- the shapes of ConvBiasAct.k13h_slower, which run cast + x * gate + rocBLAS + K10 by default, included -- unless
    the shape is in ConvBiasAct.k13h_deep_slower; everything else takes today's branch.  The armed layers' results
    differ from the library chain's by rounding (another summation order), and are the bits of K13h's other
    configurations."""
    for m in folded.modules():
        if type(m) is ConvBiasAct and m.act is None and _plain_1x1(m.conv) and m.conv.in_channels >= 768 \
                and m.conv.out_channels > 160:
            m.deep_projects = True


def _arm_expand_depthwise(folded, field='hand_to', strides=(1,), k=3):
    """fuse_expand_depthwise: every plain 1x1 ConvBiasAct that emits no mean and stands directly in front of a 3x3,
    stride-1, padding-1 DepthwiseBiasAct of as many channels without a folded ZeroPad2d -- the expand and depthwise
    layers of the stride-1 MBConv blocks: 28 pairs of EfficientNetV2-S, 59 of -L, 6 of MobileNetV3, none of ResNet-18
    -- is armed to hand its input to that layer, which runs both as ONE launch (K25h, both .last_path 'k25h') where
    DepthwiseBiasAct.k25h_takes says so: the bits of the chain K13h + K11, the expanded activation kept in LDS.  The
    chain runs everywhere else (24x24, 12x12 and 64x64 planes, the expand shapes of ConvBiasAct.k13h_slower, CPU, ...).
    The stride-2 blocks have their folded ZeroPad2d (an Identity) between the two layers and stay unarmed.
    fuse_expand_depthwise_planes arms the same pairs on `field` 'hand_planes_to' instead, for K26h ('k26h';
    DepthwiseBiasAct.k26h_takes: the 24x24 and 12x12 planes K25h leaves to the chain).
    fuse_expand_depthwise_tiles arms them on 'hand_tiles_to' with `strides` (1, 2): also the stride-2 pairs whose
    depthwise layer has padding 1, no folded ZeroPad2d and no squeeze-excite block behind it (K27h has no mean), directly
    behind the expand -- 6 + 2 pairs of MobileNetV3; the stride-2 layers of EfficientNetV2 carry a folded padding or, the
    one symmetric one of each network, emit the mean, and stay unarmed (28 of -S, 59 of -L) -- for K27h ('k27h';
    DepthwiseBiasAct.k27h_takes: the large planes of the layers without a squeeze-excite mean).
    fuse_expand_depthwise5x5 arms on 'hand_k5_to', with `k` 5 and `strides` (1, 2), the pairs whose depthwise layer is
    5x5 with padding 2 (k // 2) and no folded ZeroPad2d, a mean behind it allowed at either stride: 6 pairs of
    MobileNetV3, none of the other three networks -- for K28h ('k28h'; DepthwiseBiasAct.k28h_takes)."""
    for _, _, a, b in _adjacent_children(folded):
        expand, dw = _only_layer(a), _only_layer(b)
        if type(expand) is ConvBiasAct and not expand.emit_mean and _plain_1x1(expand.conv) \
                and isinstance(dw, DepthwiseBiasAct) and dw.k == k and dw.stride in strides and dw.pad == k // 2 \
                and (k == 5 or dw.stride == 1 or not dw.emit_mean) \
                and dw.pads is None and dw.weight.shape[0] == expand.conv.out_channels:
            setattr(expand, field, (dw,))


def _arm_split_gemm(folded):
    """split_gemm: every plain 1x1 ConvBiasAct that emits no mean -- the expand, project and head-side 1x1 layers --
    runs K20 (.last_path 'k20' / 'k20_gate'; an armed FusedMBConv block reports 'k20_pre') wherever K13 would take the
    input, unless the shape is in ConvBiasAct.k20_slower: the f32 product on the bf16 matrix cores, from operands split
    into three bf16 pieces each and the six largest of the nine cross products, with K13's prologue, gate, epilogue and
    skip.  f32-grade (it passes K13's fp64 bound) but not K13's bits.  Everything K20 refuses runs exactly today's
    branch.  The split weight is derived state, cached per weight storage and version."""
    for m in folded.modules():
        if isinstance(m, ConvBiasAct) and not m.emit_mean and _plain_1x1(m.conv):
            m.split_gemm = True


def _fuse_stem(folded):
    """fuse_stem: the stem -- the first dense 3x3 stride-2 padding-1 Cin = 3 ConvBiasAct -- becomes a StemConvBiasAct,
    which runs Preproc, the convolution and its epilogue as ONE launch (K17) where that kernel takes the input and the
    library chain everywhere else; the Preproc directly in front of it is armed to hand its input over untouched."""
    for stem_blk in _replace_conv_bias_act(folded, StemConvBiasAct, first_only=True):
        for _, _, prev, nxt in _adjacent_children(folded):
            while isinstance(nxt, nn.Sequential) and not isinstance(nxt, ConvBNAct) and len(nxt):
                nxt = nxt[0]  # (EfficientNetV2: Preproc stands in front of the `features` container)
            if isinstance(prev, Preproc) and nxt is stem_blk:
                prev.hand_to = (stem_blk[0],)


# what an option needs of (fused_epilogue, dtype), and how the error says it
_NEEDS = {'fused': (lambda fused, dtype: fused, 'fused_epilogue=True'),
          '16bit': (lambda fused, dtype: dtype is not None, 'a 16-bit copy (dtype=torch.float16 / torch.bfloat16)'),
          'f32': (lambda fused, dtype: fused and dtype is None, 'fused_epilogue=True and an f32 copy (no dtype=)')}
_OPTION_NEEDS = (('fuse_blocks', '16bit'), ('fuse_stem', 'fused'), ('block_depthwise', 'fused'),
                 ('deep_projects', '16bit'), ('winograd3x3', 'f32'), ('split_gemm', 'f32'),
                 ('strided3x3', 'f32'), ('split3x3', 'f32'), ('fuse_expand_depthwise', '16bit'),
                 ('fuse_expand_depthwise_planes', '16bit'), ('fuse_expand_depthwise_tiles', '16bit'),
                 ('fuse_expand_depthwise5x5', '16bit'))


def fold_batchnorm(backbone, fused_epilogue=False, dtype=None, fuse_blocks=False, fuse_stem=False,
                   block_depthwise=False, deep_projects=False, winograd3x3=False, split_gemm=False,
                   strided3x3=False, fuse_expand_depthwise=False, fuse_expand_depthwise_planes=False,
                   fuse_expand_depthwise_tiles=False, split3x3=False, fuse_expand_depthwise5x5=False):
    """Inference-time copy of `backbone` with every batch norm folded into the convolution in front
    of it (w' = w * gamma / sqrt(var + eps), b' = beta - mean * gamma / sqrt(var + eps)): the same
    function up to rounding (features equal to ~1e-5 relative in f32), one elementwise pass over
    every activation less.  EfficientNetV2-S forward at the bench shape: 13.3 -> 11.8 ms in f32,
    11.6 -> 10.2 ms under f16 autocast (tools/experiments/bn_backend_probe.py).  The original keeps
    its checkpoint-compatible parameters; the copy has conv biases and no BatchNorm2d.
    fused_epilogue=True additionally runs "+ bias, activation" behind each folded convolution as one
    in-place HIP pass (ConvBiasAct) instead of PyTorch-ROCm's two elementwise kernels, folds the explicit paddings into
    the depthwise kernels (_fold_paddings), wires the squeeze-excite blocks to the layers around them
    (_wire_squeeze_excite) and, on an f32 copy, arms the FusedMBConv blocks for the K13 prologue (_arm_pre_pairs).
    dtype=torch.float16 / torch.bfloat16 (needs fused_epilogue=True) returns a 16-bit inference copy (_cast_16bit).
    The options, all off by default; each step's docstring says what it arms.  None adds a module, a buffer or a
    state_dict key to the copy without it:
    fuse_blocks=True (needs a 16-bit dtype): FusedMBConv blocks as one launch, K16h (_arm_fused_pairs).
    fuse_stem=True (needs fused_epilogue=True; any dtype): Preproc and the stem as one launch, K17 (_fuse_stem).
    block_depthwise=True (needs fused_epilogue=True; any dtype): K18 where K11 would take its generic kernel
    (_arm_block_depthwise).
    deep_projects=True (needs a 16-bit dtype): the deep project convolutions on K13h's deep-K configuration
    (_arm_deep_projects).
    winograd3x3=True, strided3x3=True, split3x3=True (each needs fused_epilogue=True and an f32 copy, i.e. no dtype --
    K14h serves the 16-bit copies): the dense 3x3 layers on the kernels of DENSE3X3_KERNELS (_replace_dense3x3) --
    stride 1 with Cin % 4 == 0 as Winograd on the f32 MFMA, K19; stride 2 with Cin % 4 == 0 as an implicit GEMM on
    the f32 MFMA, K22; stride 1 with Cin % 8 == 0 on the bf16 matrix cores by operand split, K21.  With split3x3 and
    winograd3x3 both on the layers are SplitConv3x3BiasAct and run K21 where it takes the tensor, K19 where K21 refuses
    or lists the shape and K19 takes it, the library path otherwise.
    split_gemm=True (needs fused_epilogue=True and an f32 copy): the f32 1x1 layers on K20 (_arm_split_gemm).
    fuse_expand_depthwise=True (needs a 16-bit dtype): the 1x1 expand and the stride-1 depthwise 3x3 layer of an MBConv
    block as one launch, K25h (_arm_expand_depthwise).
    fuse_expand_depthwise_planes=True (needs a 16-bit dtype): the same pairs as one launch on the planes K25h refuses
    (24x24, 12x12: 384 px inputs), K26h (_arm_expand_depthwise on hand_planes_to).
    fuse_expand_depthwise_tiles=True (needs a 16-bit dtype): the same pairs and the stride-2 pairs without a folded
    padding as one launch on the large planes of the layers that emit no mean (64x64, 128x128 -> 64x64, 32x32 -> 16x16 of
    MobileNetV3), K27h (_arm_expand_depthwise on hand_tiles_to).
    fuse_expand_depthwise5x5=True (needs a 16-bit dtype): the 1x1 expand and the depthwise 5x5 layer of stride 1 or 2 of an
    MBConv block as one launch, with the squeeze-excite mean, K28h (_arm_expand_depthwise on hand_k5_to with k = 5: the six
    5x5 blocks of MobileNetV3).
    The options of one family combine freely (f32: fuse_stem, block_depthwise, winograd3x3, split_gemm, strided3x3, split3x3; 16-bit:
    fuse_blocks, fuse_stem, block_depthwise, deep_projects, fuse_expand_depthwise, fuse_expand_depthwise_planes, fuse_expand_depthwise_tiles, fuse_expand_depthwise5x5): no two of them arm the same field of the same module, and
    each unit of a copy with several options on returns the bits of the copy with that unit's options alone (DESIGN.md
    section 24).  The order of the steps below matters: the references between modules are plain attributes, and a
    module replaced after one was taken leaves it pointing at an object outside the tree.  pre_pair, fused_pair and
    hand_to are taken after the replacements (Dense3x3BiasAct's classes, Conv3x3BiasAct, StemConvBiasAct); mean_from and
    gate_to before them, at layers no replacement touches in these networks (those that emit a mean; the 1x1 projects).
    tests/test_backbone_option_combos_host.py checks every reference of every combination."""
    import copy
    if backbone.training:
        raise ValueError('fold_batchnorm needs the running statistics of an eval-mode network')
    if dtype not in (None,) + _16BIT:
        raise ValueError(f'fold_batchnorm: dtype must be None, torch.float16 or torch.bfloat16, got {dtype}')
    if dtype is not None and not fused_epilogue:
        raise ValueError('fold_batchnorm: a 16-bit copy (dtype=) needs fused_epilogue=True')
    options = dict(fuse_blocks=fuse_blocks, fuse_stem=fuse_stem, block_depthwise=block_depthwise,
                   deep_projects=deep_projects, winograd3x3=winograd3x3, split_gemm=split_gemm,
                   strided3x3=strided3x3, fuse_expand_depthwise=fuse_expand_depthwise,
                   fuse_expand_depthwise_planes=fuse_expand_depthwise_planes,
                   fuse_expand_depthwise_tiles=fuse_expand_depthwise_tiles, split3x3=split3x3,
                   fuse_expand_depthwise5x5=fuse_expand_depthwise5x5)
    for option, need in _OPTION_NEEDS:
        met, text = _NEEDS[need]
        if options[option] and not met(fused_epilogue, dtype):
            raise ValueError(f'fold_batchnorm: {option}=True needs {text}')
    folded = copy.deepcopy(backbone)
    _fold_convs(folded, fused_epilogue)
    if fused_epilogue:
        _fold_paddings(folded)
        _wire_squeeze_excite(folded)
    _replace_dense3x3(folded, options)
    if fused_epilogue and dtype is None:
        _arm_pre_pairs(folded)
    if dtype is not None:
        _cast_16bit(folded, dtype)
    if fuse_blocks:
        _arm_fused_pairs(folded)
    if block_depthwise:
        _arm_block_depthwise(folded)
    if deep_projects:
        _arm_deep_projects(folded)
    if split_gemm:
        _arm_split_gemm(folded)
    if fuse_expand_depthwise:
        _arm_expand_depthwise(folded)
    if fuse_expand_depthwise_planes:
        _arm_expand_depthwise(folded, 'hand_planes_to')
    if fuse_expand_depthwise_tiles:
        _arm_expand_depthwise(folded, 'hand_tiles_to', strides=(1, 2))
    if fuse_expand_depthwise5x5:
        _arm_expand_depthwise(folded, 'hand_k5_to', strides=(1, 2), k=5)
    if fuse_stem:
        _fuse_stem(folded)
    return folded


def calibrate_batchnorm(backbone, res, dev, batches=2, batch_size=16, seed=7, samples=None):
    """Random-weight networks with untouched BatchNorm statistics (mean 0 / var 1) let activations
    grow layer by layer until they overflow.  A few forward passes in training mode on synthetic
    crops set the running statistics (cumulative average), which keeps every layer at unit scale --
    the regime a trained checkpoint is in.  Weights stay random; the FLOPs are unchanged.
    samples: optional f32 crops [n, 3, res, res] of the kind the network will actually see (the
    benchmark's sampler output: low-contrast resampled noise with zero padding, whose statistics
    differ enough from uniform noise for an f16 EfficientNetV2-L to overflow); they are used in
    chunks of batch_size beside the uniform-noise batches."""
    bns = [m for m in backbone.modules() if isinstance(m, torch.nn.BatchNorm2d)]
    for m in bns:
        m.momentum = None
        m.reset_running_stats()
    backbone.train()
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for _ in range(batches):
            backbone(torch.rand(batch_size, 3, res, res, device=dev, generator=g))
        if samples is not None:
            for chunk in samples.float().split(batch_size):
                if len(chunk) > 1:
                    backbone(chunk)
    backbone.eval()
    return backbone
