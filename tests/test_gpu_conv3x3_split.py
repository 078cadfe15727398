"""GPU: K21 (csrc/conv3x3_split.hip), the dense 3x3 stride-1 convolution of the f32 inference copy on the bf16 matrix
cores by operand split, with the K10 epilogue, through the C-ABI wrapper (kernels.conv3x3_bias_act_split).

The fp64 bound (_check), every element:

    |got - ref| <= 1.1 (54 Cp + 4) 2^-24 S + 1e-6 |ref| + 2^-24

ref is F.conv2d(x.double(), w.double(), b.double(), 1, 1) through activation and skip, Cp is Cin rounded up to the
kernel's chunk of 16, S = F.conv2d(|x|, |w|, padding 1) in fp64 + |bias|.  Derivation: a sum of the 6 * 9 * Cp piece
products in any order has fewer than 54 Cp additions, each of which rounds a partial sum of magnitude at most S (this
covers the unknown order inside one MFMA); "+ bias" adds one rounding; the three dropped products are at most
(2 + 2^-8) 2^-24 |w v| each way, summed to under 3 * 2^-24 S: (54 Cp + 4) 2^-24 S in all.  The activation's Lipschitz
constant is at most 1.1 (silu 1.0998); 1e-6 |ref| covers the activation's own evaluation and the rounding of the skip's
addition; 2^-24 is absolute slack below the smallest bias scale.  It is a worst-case bound: it catches a missed tap,
not one missed piece product at large Cin -- that is what the exact-integer cases are for.

Also: accuracy as a ratio to the library's f32 convolution, determinism (calls, a sliced batch, a graph replay, the
skip being x itself), a NaN guard band, the SplitConv3x3BiasAct module inside the copies (paths, switches, refusals,
the combination with winograd3x3), whole-backbone accuracy against an fp64 forward, the loader and the API, and a copy
with every f32 option on."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases
from test_conv3x3_split_host import INT_SHAPES, integer_case, magnitude_sum

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
CHUNK = 16


def _inputs(B, K, M, H, W, seed, residual, border=1.0):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    if border != 1.0:   # large border pixels: a wrong halo (a missed or a doubled edge tap) shows
        edge = torch.ones(H, W, device='cuda')
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
        x = x * edge
    w = torch.randn(M, K, 3, 3, device='cuda', generator=g) / (9 * K) ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    r = torch.randn(B, M, H, W, device='cuda', generator=g) if residual else None
    return x, w, b, r


def _ref64(x, w, b, act, r):
    ref = _TORCH_ACT[act](F.conv2d(x.double(), w.double(), b.double(), 1, 1))
    return ref if r is None else ref + r.double()


def _reference(x, w, b, act, r):
    """(fp64 result, the bound of the module docstring)."""
    K = x.shape[1]
    Cp = (K + CHUNK - 1) // CHUNK * CHUNK
    ref = _ref64(x, w, b, act, r)
    S = F.conv2d(x.double().abs(), w.double().abs(), None, 1, 1) + b.double().abs()[None, :, None, None]
    return ref, 1.1 * (54 * Cp + 4) * 2.0 ** -24 * S + 1e-6 * ref.abs() + 2.0 ** -24


def _check(x, w, b, act, r, got):
    """The bound of the module docstring, on every element."""
    ref, bound = _reference(x, w, b, act, r)
    assert got.shape == ref.shape and got.dtype == torch.float32
    err = (got.double() - ref).abs()
    print(f'k21 check {tuple(x.shape)} -> {tuple(got.shape)} {act} skip {r is not None}: '
          f'max err / bound = {float((err / bound).max()):.4f}')
    excess = float((err - bound).max())
    assert excess <= 0, excess


def _run(x, w, b, act, r, **kw):
    from metrabs_amd import kernels
    ws = kernels.pack_conv3x3_split_weight(w)
    assert kernels.conv3x3_split_supported(x, ws), tuple(x.shape)
    return kernels.conv3x3_bias_act_split(x, ws, b, act, residual=r, **kw)


# (B, Cin, Cout, H, W, the activation that runs with the skip): one partial tile; a partial chunk and several images;
# odd H and a partial position fragment; past a channel block; a tall plane; many chunks
EDGE_CASES = [(1, 8, 5, 4, 4, None), (3, 24, 96, 16, 24, 'relu'), (2, 40, 40, 5, 36, 'silu'),
              (2, 64, 130, 8, 16, 'hardswish'), (1, 8, 16, 72, 8, 'silu'), (1, 136, 260, 4, 64, 'relu')]


@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('case', EDGE_CASES)
def test_k21_every_epilogue_and_edge_geometry(act, case, hip_lib):
    """The four activations on every geometry; the skip on once and off three times per geometry."""
    B, K, M, H, W, skip_act = case
    x, w, b, r = _inputs(B, K, M, H, W, 7, act == skip_act, border=8.0)
    _check(x, w, b, act, r, _run(x, w, b, act, r))


@functools.lru_cache(maxsize=None)
def _armed_shapes(name, res):
    """(Cin, Cout, H, W, act, residual) of every armed layer's input at `res` px, from a hooked forward."""
    from metrabs_amd import backbones
    S3 = backbones.SplitConv3x3BiasAct
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True, split3x3=True).cuda()
    shapes = set()

    def hook(mod, args, kwargs):
        x = args[0]
        shapes.add((x.shape[1], mod.conv.out_channels, x.shape[2], x.shape[3], mod.act_name,
                    kwargs.get('residual') is not None))

    hs = [m.register_forward_pre_hook(hook, with_kwargs=True) for m in net.modules() if isinstance(m, S3)]
    assert hs
    S3.use_k21 = False
    try:
        with torch.inference_mode():
            net(torch.rand(1, 3, res, res, device='cuda'))
    finally:
        S3.use_k21 = True
    for h in hs:
        h.remove()
    return tuple(sorted(shapes, key=str))


@pytest.mark.parametrize('name,res', [('efficientnetv2-s', 256), ('efficientnetv2-s', 224), ('efficientnetv2-l', 384),
                                      ('resnet18', 256)])
def test_k21_matches_fp64_on_every_armed_shape(name, res, hip_lib):
    shapes = _armed_shapes(name, res)
    assert len(shapes) >= 3, shapes
    for i, (K, M, H, W, act, res_) in enumerate(shapes):
        x, w, b, r = _inputs(1, K, M, H, W, 2000 + i, res_)
        _check(x, w, b, act, r, _run(x, w, b, act, r))


@pytest.mark.parametrize('skip', [False, True])
@pytest.mark.parametrize('kind', ['a', 'b', 'c'])
@pytest.mark.parametrize('shape', INT_SHAPES)
def test_k21_is_exact_on_integers_that_need_every_piece(shape, kind, skip, hip_lib):
    """The cases of test_conv3x3_split_host.integer_case: every piece product and every partial sum is an integer
    below 2^24 (asserted on S), so the six bf16 products and the f32 accumulation are exact and the result must equal
    the fp64 convolution -- a dropped product, a swapped tap, a transposed fragment or a wrong halo cannot hide in
    rounding."""
    x, w, b, r = (t.cuda() for t in integer_case(kind, shape))
    r = r if skip else None
    S = magnitude_sum(x, w, b)
    assert S.max() < 2 ** 24
    ref = _ref64(x, w, b, None, r)
    assert float(ref.abs().max()) < 2 ** 24
    assert torch.equal(_run(x, w, b, None, r), ref.float())


@functools.lru_cache(maxsize=None)
def _pinned_library_error(B, K, M, H, W):
    """Relative RMS error against fp64 of K21 and of the library's f32 convolution (deterministic solvers), same
    tensors."""
    x, w, b, _ = _inputs(B, K, M, H, W, 11, False)
    ref = _ref64(x, w, b, None, None)
    with _pinned():
        lib = F.conv2d(x, w, b, 1, 1)
    got = _run(x, w, b, None, None)
    rel = lambda t: float((t.double() - ref).norm() / ref.norm())
    return rel(got), rel(lib)


@pytest.mark.parametrize('shape', [(3, 24, 24, 32, 32), (3, 64, 256, 8, 8), (3, 512, 64, 8, 8)])
def test_k21_accuracy_is_within_twice_the_librarys(shape, hip_lib):
    """The gate of 2 is K20's: both are f32 rounding noise of different summation orders."""
    e_k21, e_lib = _pinned_library_error(*shape)
    print(f'k21 accuracy {shape}: relative RMS error against fp64: K21 {e_k21:.4g}, library {e_lib:.4g}, '
          f'ratio {e_k21 / e_lib:.3f}')
    assert e_k21 <= 2 * e_lib, (e_k21, e_lib)


def test_k21_is_deterministic_and_graph_safe(hip_lib):
    from metrabs_amd import kernels
    for (B, K, M, H, W, res_) in [(3, 24, 24, 32, 32, True), (3, 48, 192, 16, 16, False), (3, 40, 40, 5, 36, True)]:
        x, w, b, r = _inputs(B, K, M, H, W, 3, res_)
        ws = kernels.pack_conv3x3_split_weight(w)
        a = kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=r)
        assert torch.equal(a, kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=r))
        # image 1 of 3 as a batch of its own: other workgroups, the same bits
        part = kernels.conv3x3_bias_act_split(x[1:2], ws, b, 'silu', residual=None if r is None else r[1:2])
        assert torch.equal(part, a[1:2])
        if K == M:   # the skip being x itself (the stage-1 blocks) or a copy of it
            assert torch.equal(kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=x),
                               kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=x.clone()))
        with torch.inference_mode():
            out = torch.empty_like(a)
            assert kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=r, out=out) is out
            assert torch.equal(out, a)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=r, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.conv3x3_bias_act_split(x, ws, b, 'silu', residual=r, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


@pytest.mark.parametrize('shape', [(8, 5, 4, 4), (40, 40, 5, 36), (64, 130, 8, 16)])
def test_k21_writes_nothing_outside_y_and_reads_nothing_outside_its_inputs(shape, hip_lib):
    """Nothing outside y is written (conv_fuzz.guarded_out / bands_intact), and with x and the skip carved out of a
    buffer filled with NaN no NaN gets into y: a read outside x or the skip that reached a stored value would bring
    one in."""
    import conv_fuzz
    from metrabs_amd import kernels
    K, M, H, W = shape
    B = 3
    x0, w, b, r0 = _inputs(B, K, M, H, W, 5, True, border=8.0)
    nx, ny, gap = x0.numel(), r0.numel(), 1024
    buf = torch.full((3 * gap + nx + ny,), float('nan'), device='cuda')
    ox, orr = gap, 2 * gap + nx
    x, r = buf[ox:ox + nx].view_as(x0), buf[orr:orr + ny].view_as(r0)
    x.copy_(x0), r.copy_(r0)
    before = buf.view(torch.int32).clone()
    ws = kernels.pack_conv3x3_split_weight(w)
    store, y = conv_fuzz.guarded_out((B, M, H, W), torch.float32, 'cuda')
    assert kernels.conv3x3_bias_act_split(x, ws, b, 'relu', residual=r, out=y) is y
    torch.cuda.synchronize()
    assert conv_fuzz.bands_intact(store)
    assert torch.equal(buf.view(torch.int32), before)
    assert not torch.isnan(y).any()
    _check(x0, w, b, 'relu', r0, y)
    assert torch.equal(y, kernels.conv3x3_bias_act_split(x0, ws, b, 'relu', residual=r0))


def test_k21_wrapper_argument_checks(hip_lib):
    from metrabs_amd import kernels
    x, w, b, r = _inputs(2, 8, 16, 16, 16, 1, True)
    ws = kernels.pack_conv3x3_split_weight(w)
    ok = kernels.conv3x3_bias_act_split(x, ws, b, None, residual=r)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x.half(), ws, b, None)                        # dtype
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, ws.float(), b, None)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x.to(memory_format=torch.channels_last), ws, b, None)   # layout
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, w, b, None)                                # the OIHW weight
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, torch.cat([ws, ws], dim=4), b, None)       # another Cin
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, ws, b[:4], None)
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, ws, b, None, residual=r[:, :, :4].contiguous())
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, ws, b, None, residual=r.half())
    with pytest.raises(ValueError):
        kernels.conv3x3_bias_act_split(x, ws, b, None, residual=r, out=r)            # an aliasing out
    with pytest.raises(RuntimeError):                                                # no CPU fallback
        kernels.conv3x3_bias_act_split(x.cpu(), ws.cpu(), b.cpu(), None)
    with pytest.raises(RuntimeError):                                                # MTR_E_SHAPE through check()
        kernels.conv3x3_bias_act_split(x[:, :, :, :6].contiguous(), ws, b, None)
    assert kernels.conv3x3_split_supported(x, ws)
    assert kernels.conv3x3_split_supported(x[:, :, :7].contiguous(), ws)             # odd H is taken
    assert not kernels.conv3x3_split_supported(x[:, :, :, :6].contiguous(), ws)      # W % 4 != 0
    assert not kernels.conv3x3_split_supported(x.to(memory_format=torch.channels_last), ws)
    assert not kernels.conv3x3_split_supported(x.half(), ws)
    assert not kernels.conv3x3_split_supported(x, w)
    flat = torch.zeros(x.numel() + 2, device='cuda')
    assert not kernels.conv3x3_split_supported(flat[2:].view_as(x), ws)              # 8 bytes past a boundary
    assert torch.equal(ok, kernels.conv3x3_bias_act_split(x, ws, b, None, residual=r))


def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _pinned():
    return torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True)


def _all_paths(net):
    return [getattr(m, 'last_path', None) for m in net.modules()]


@functools.lru_cache(maxsize=None)
def _backbone_128(name):
    """One calibrated backbone, its default, armed and winograd3x3 copies, an input, the default copy's features under
    the deterministic pin and the fp64 CPU forward of the same folded network: made once, left unchanged."""
    import copy
    from metrabs_amd import backbones
    net = _calibrated(name, 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, split3x3=True)
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(4))
    with torch.inference_mode():
        want = copy.deepcopy(plain).cpu().double()(x.cpu().double())
        with _pinned():
            ref = plain(x).clone()
    return net, plain, armed, x, ref, want


def test_armed_efficientnet_takes_k21_where_it_applies(hip_lib):
    from metrabs_amd import backbones
    S3 = backbones.SplitConv3x3BiasAct
    _, plain, armed, x, ref, _ = _backbone_128('efficientnetv2-s')
    feats = armed[1]
    mods = [m for m in armed.modules() if isinstance(m, S3)]
    assert len(mods) == 8 and 'k21' not in _all_paths(plain)
    with torch.inference_mode(), _pinned():
        on = armed(x).clone()
        assert [m.last_path for m in mods] == ['k21'] * 8
        # stage 1: plain 3x3 blocks whose skip K21 adds; stages 2 - 3: a stride-2 first block, then armed expands
        for blk in feats[1]:
            assert isinstance(blk.block[0][0], S3) and blk.last_path is None
        for stage in (feats[2], feats[3]):
            assert stage[0].last_path == 'k13_pre'
            for blk in list(stage)[1:]:
                assert blk.last_path == 'k21' and blk.pre_pair[0] in mods and blk.pre_pair[1].last_path == 'k13'
        assert torch.isfinite(on).all() and not torch.equal(on, ref)
        rel = float((on - ref).norm() / ref.norm())
        print(f'armed vs default copy, EfficientNetV2-S 128 px: relative difference {rel:.3g}')
        assert rel < 1e-4
        # a stage-1 block: the layer's own call with the block's input as the skip
        blk = feats[1][0]
        xin = torch.randn(2, 24, 64, 64, device='cuda')
        layer = blk.block[0][0]
        assert blk.residual and torch.equal(blk(xin), layer(xin, residual=xin)) and layer.last_path == 'k21'
        got = blk(xin)
        _check(xin, layer.conv.weight, layer.bias, layer.act_name, xin, got)
        # the switch, and a listed shape: exactly what the default copy runs, the same bits
        shipped = S3.k21_slower
        try:
            S3.use_k21 = False
            off = armed(x).clone()
            assert all(m.last_path == 'library' for m in mods) and 'k21' not in _all_paths(armed)
            assert all(b_.last_path == 'k13_pre' for st_ in (feats[2], feats[3]) for b_ in st_)
            assert torch.equal(off, ref)
            S3.use_k21 = True
            S3.k21_slower = frozenset({(48, 192, 32, 32)})
            armed(x)
            assert all(b_.last_path == 'k13_pre' for b_ in feats[2]) and feats[3][1].last_path == 'k21'
            assert feats[2][1].pre_pair[0].last_path == 'library'
        finally:
            S3.use_k21, S3.k21_slower = True, shipped
        # autocast and a channels_last input: the library path
        with torch.autocast('cuda', dtype=torch.float16):
            armed(x)
        assert all(m.last_path == 'library' for m in mods)
        armed(x)
        assert all(m.last_path == 'k21' for m in mods)
        m0 = mods[0]
        assert m0.k21_takes(xin) and not m0.k21_takes(xin.to(memory_format=torch.channels_last))
        assert m0.path(xin) == 'k21' and m0.path(xin.to(memory_format=torch.channels_last)) == 'library'
        m0(xin.to(memory_format=torch.channels_last))
        assert m0.last_path == 'library'
        m0(xin)
        assert m0.last_path == 'k21'
        assert not m0.k21_takes(xin[:, :, :, :62].contiguous())                        # W % 4 != 0
        assert m0.k21_takes(xin[:, :, :63].contiguous())                               # an odd H is taken
    xg = torch.rand(2, 24, 64, 64, device='cuda', requires_grad=True)   # a gradient wanted: the library path
    assert not mods[0].k21_takes(xg) and mods[0].path(xg) == 'library'


def test_with_winograd3x3_a_listed_shape_runs_k19_with_the_winograd_copys_bits(hip_lib):
    from metrabs_amd import backbones
    S3 = backbones.SplitConv3x3BiasAct
    net, _, _, x, _, _ = _backbone_128('efficientnetv2-s')
    wino = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True)
    both = backbones.fold_batchnorm(net, fused_epilogue=True, winograd3x3=True, split3x3=True)
    mods = [m for m in both.modules() if isinstance(m, S3)]
    shipped = S3.k21_slower
    try:
        with torch.inference_mode(), _pinned():
            both(x)
            assert [m.last_path for m in mods] == ['k21'] * 8
            # every armed shape listed: the winograd3x3-only copy, bit for bit
            S3.k21_slower = frozenset({(24, 24, 64, 64), (48, 192, 32, 32), (64, 256, 16, 16)})
            got, want = both(x).clone(), wino(x).clone()
            assert [m.last_path for m in mods] == ['k19'] * 8
            assert [p for p in _all_paths(both) if p] == [p for p in _all_paths(wino) if p]
            assert torch.equal(got, want)
            # one listed shape: that tensor runs K19, the others K21
            S3.k21_slower = frozenset({(48, 192, 32, 32)})
            both(x)
            assert both[1][2][1].last_path == 'k19' and both[1][3][1].last_path == 'k21'
            layer = both[1][2][1].pre_pair[0]
            xin = torch.randn(2, 48, 32, 32, device='cuda')
            twin = wino[1][2][1].pre_pair[0]
            assert layer.path(xin) == 'k19' and torch.equal(layer(xin), twin(xin))
    finally:
        S3.k21_slower = shipped


@pytest.mark.parametrize('name', ['efficientnetv2-s', 'resnet18'])
def test_whole_backbone_accuracy_against_fp64(name, hip_lib):
    """The armed copy's features against an fp64 CPU forward of the same folded network: a relative RMS error of at
    most 2 x the default copy's against that same forward -- both are rounding noise from different summation orders,
    hence the margin (the criterion of DESIGN.md sections 22 - 24)."""
    _, plain, armed, x, ref, want = _backbone_128(name)
    with torch.inference_mode(), _pinned():
        got_armed = armed(x).double().cpu()
    assert 'k21' in _all_paths(armed)
    rel = lambda t: float((t - want).norm() / want.norm())
    e_plain, e_armed = rel(ref.double().cpu()), rel(got_armed)
    print(f'{name} 128 px B = 2, relative RMS error against fp64: default copy {e_plain:.4g}, '
          f'armed copy {e_armed:.4g}')
    assert e_armed <= 2 * e_plain, (e_armed, e_plain)


def _model_dir(tmp_path):
    from metrabs_amd import backbones, loading
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    raw = dict(proc_side=256, stride_train=32, stride_test=32, centered_stride=True, depth=8,
               box_size_mm=2200, efficientnet_size='s', weak_perspective=False, mix_3d_inside_fov=0.5)
    bb = backbones.efficientnetv2('s')
    model = Metrabs(bb, JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(raw),
                    in_channels=bb.out_channels)
    model.load_state_dict(cases.deterministic_state(model.state_dict(), seed=11))
    skel = {'': dict(indices=list(range(17)), names=cases.COCO17, edges=cases.COCO17_EDGES)}
    d = str(tmp_path / 'model')
    loading.save_model_dir(d, model, raw, skel, np.eye(17, dtype=np.float32))
    return d


def _api_inputs(seed=5):
    images = torch.stack([cases.synth_images(1, 240, 320, seed + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    return images, boxes


def _poses(est, images, boxes, num_aug=1):
    with torch.inference_mode():
        r = est.estimate_poses_batched(images, boxes, num_aug=num_aug)
    return torch.cat(r['poses3d']).clone()


class _Fp64Backbone(torch.nn.Module):
    """A folded backbone evaluated in fp64 on the CPU, handing f32 features back: the truth of the API test."""

    def __init__(self, folded):
        super().__init__()
        import copy
        # (in a tuple: not a registered submodule, so the estimator still finds its crop model's parameters on the GPU)
        self._net = (copy.deepcopy(folded).cpu().double(),)

    def forward(self, x):
        return self._net[0](x.detach().double().cpu()).float().to(x.device)


def test_k21_through_the_loader_and_the_api(tmp_path, hip_lib):
    """Three crops through estimate_poses_batched.  A graphed call of the armed model returns the eager call's bits, and
    MPJPE(armed, fp64) <= 2 x MPJPE(default copy, fp64), the reference being the same folded network with its backbone
    evaluated in fp64 on the CPU (sampler and head are the same kernels for every arm): both are f32 rounding noise
    from different summation orders.  A wrong armed layer moves the features by far more."""
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    plain = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
    truth.crop_model.backbone = _Fp64Backbone(truth.crop_model.backbone)
    est = loading.load_multiperson_model(d, split3x3=True)
    eager = loading.load_multiperson_model(d, split3x3=True)
    for m in (plain, est, eager):
        m.crop_model.deterministic_backbone = True
    est.graph_batches, eager.graph_batches, truth.graph_batches = True, False, False
    images, boxes = _api_inputs(5)
    p_armed, p_graph = _poses(eager, images, boxes), _poses(est, images, boxes)
    assert torch.isfinite(p_armed).all()
    assert torch.equal(p_armed, p_graph), float((p_armed - p_graph).abs().max())
    for model in (est, eager):
        paths = [m.last_path for m in model.crop_model.backbone.modules()
                 if isinstance(m, backbones.SplitConv3x3BiasAct)]
        assert paths == ['k21'] * 8, paths
    p_true, p_plain = _poses(truth, images, boxes), _poses(plain, images, boxes)
    assert 'k21' not in _all_paths(plain.crop_model.backbone)
    assert p_true.shape == p_armed.shape and torch.isfinite(p_true).all()
    mpjpe = lambda p, q: float((p - q).norm(dim=-1).mean())
    e_armed, e_plain = mpjpe(p_armed, p_true), mpjpe(p_plain, p_true)
    print(f'MPJPE to the fp64-backbone poses: armed copy {e_armed:.5g} mm, default copy {e_plain:.5g} mm; '
          f'mean |p| {float(p_true.norm(dim=-1).mean()):.4g} mm')
    assert 0 < e_armed <= 2 * e_plain, (e_armed, e_plain)


def test_every_f32_option_on_runs_k21_on_every_stride_1_3x3_layer(hip_lib):
    """EfficientNetV2-S at 128 px, B = 2, folded with fuse_stem, block_depthwise, winograd3x3, split_gemm, strided3x3
    and split3x3, k21_slower emptied: every dense 3x3 stride-1 layer reports 'k21', the forward is finite and within
    the 2 x gate against the fp64 forward."""
    from metrabs_amd import backbones
    S3 = backbones.SplitConv3x3BiasAct
    net, _, _, x, ref, want = _backbone_128('efficientnetv2-s')
    every = backbones.fold_batchnorm(net, fused_epilogue=True, fuse_stem=True, block_depthwise=True, winograd3x3=True,
                                     split_gemm=True, strided3x3=True, split3x3=True)
    shipped = S3.k21_slower
    try:
        S3.k21_slower = frozenset()
        with torch.inference_mode(), _pinned():
            y = every(x).clone()
            assert torch.equal(every(x), y)
    finally:
        S3.k21_slower = shipped
    layers = [m for m in every.modules() if isinstance(m, backbones.ConvBiasAct) and m.conv.kernel_size == (3, 3)
              and m.conv.stride == (1, 1) and m.conv.groups == 1]
    assert len(layers) == 8 and all(type(m) is S3 and m.last_path == 'k21' for m in layers)
    paths = [p for p in _all_paths(every) if p is not None]
    assert 'library' not in paths and 'k19' not in paths and 'k22' in paths and 'k17' in paths
    assert torch.isfinite(y).all()
    rel = lambda t: float((t.double().cpu() - want).norm() / want.norm())
    e_plain, e_every = rel(ref), rel(y)
    print(f'every f32 option on: relative RMS error against fp64 {e_every:.4g}, default copy {e_plain:.4g}')
    assert e_every <= 2 * e_plain, (e_every, e_plain)
