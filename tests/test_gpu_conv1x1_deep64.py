"""GPU: K13's 64 x 64 ring-staged configuration 'deep64' (csrc/conv1x1.hip, code 5 of mtr_conv1x1_bias_act_pre): against an
fp64 torch evaluation, against 'tall' and 'auto' bit for bit, with and without the input prologue, guard bands, repeat
calls, graph replay, base-pointer alignment, the refusals of the entry; and the folded EfficientNetV2-S forward."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
# (K, M, H, W).  k-tiles of 32 in a ring of three, 64 x 64 tiles: one partial k-tile (fewer tiles than stages); two whole
# tiles; exactly three tiles and M past one row tile; a k tail of 4 and M = 2.5 row tiles; five tiles with a tail and
# tiles spanning 16 images; the shape the configuration was built for; and (not in the list the configuration was
# specified with) the smallest K whose whole tiles give one trip through the loop of walked, unclamped loads: five
# whole tiles and a tail
SHAPES = [(8, 8, 2, 2), (64, 64, 4, 4), (96, 72, 8, 8), (100, 160, 4, 4), (132, 200, 2, 2), (1536, 256, 8, 8),
          (164, 40, 4, 4)]


def _inputs(B, K, M, H, W, seed, gate, residual, pre):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g)
    w = torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    gt = torch.rand(B, K, device='cuda', generator=g) if gate else None
    r = torch.randn(B, M, H, W, device='cuda', generator=g) if residual else None
    bi = 0.5 * torch.randn(K, device='cuda', generator=g) if pre else None
    return x, w, b, gt, r, bi


def _check(x, w, b, act, gt, r, got):
    """The bound tests/test_gpu_conv1x1_deepk.py derives: |got - fp64| <= a small multiple of 2^-23 * sum_k |w x| (the
    f32 MFMA is an fmaf chain), through the activation (Lipschitz <= 1.1 for every act here) plus its own f32 rounding.
    x is the f32 input of the GEMM (behind the prologue, where there is one)."""
    xg = x if gt is None else x * gt[:, :, None, None]        # f32, rounded as torch's x * g
    wd = w.double().flatten(1)
    z = torch.einsum('mk,bkhw->bmhw', wd, xg.double()) + b.double()[None, :, None, None]
    s = torch.einsum('mk,bkhw->bmhw', wd.abs(), xg.double().abs()) + b.double().abs()[None, :, None, None]
    ref = _TORCH_ACT[act](z)
    if r is not None:
        ref = ref + r.double()
    bound = 4 * 2.0 ** -23 * 1.1 * s + 1e-6 * ref.abs() + 1e-30
    assert got.shape == ref.shape and got.dtype == torch.float32
    excess = float(((got.double() - ref).abs() - bound).max())
    assert excess <= 0, excess


@pytest.mark.parametrize('pre', [False, True])
@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('residual', [False, True])
@pytest.mark.parametrize('B', [1, 3])
@pytest.mark.parametrize('shape', SHAPES)
def test_deep64_matches_fp64_tall_and_auto(shape, B, residual, gate, pre, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, gt, r, bi = _inputs(B, K, M, H, W, 23 + B, gate, residual, pre)
    kw = dict(gate=gt, residual=r, in_bias=bi, in_act='silu' if pre else None)
    # the f32 tensor K10 would have left in x: what the prologue must reproduce bit for bit
    xin = kernels.bias_act_(x.clone(), bi, 'silu') if pre else x
    held = [t.clone() for t in (x, w, b) + tuple(t for t in (gt, r, bi) if t is not None)]
    G = 256   # floats: the guarded output stays 16-byte aligned
    n = B * M * H * W
    big = torch.full((n + 2 * G,), -7.0, device='cuda')
    out = big[G:G + n].view(B, M, H, W)
    assert kernels.conv1x1_plan(M, K, H * W, B, 'deep64') == ('deep64', 2, 64, 64)
    for act in ACTS:
        out.fill_(-7.0)
        got = kernels.conv1x1_bias_act(x, w, b, act, out=out, config='deep64', **kw)
        torch.cuda.synchronize()
        assert got is out
        assert bool((big[:G] == -7.0).all()) and bool((big[G + n:] == -7.0).all()), act
        _check(xin, w, b, act, gt, r, out)
        assert torch.equal(kernels.conv1x1_bias_act(x, w, b, act, config='tall', **kw), out), act
        assert torch.equal(kernels.conv1x1_bias_act(x, w, b, act, config='auto', **kw), out), act
    for t, t0 in zip((x, w, b) + tuple(t for t in (gt, r, bi) if t is not None), held):
        assert torch.equal(t, t0)   # the inputs are read only


@pytest.mark.parametrize('pre', [False, True])
@pytest.mark.parametrize('shape', [(1536, 256, 8, 8), (132, 200, 2, 2)])
def test_deep64_repeats_itself_and_replays(shape, pre, hip_lib):
    from metrabs_amd import kernels
    K, M, H, W = shape
    x, w, b, gt, r, bi = _inputs(3, K, M, H, W, 3, True, True, pre)
    kw = dict(gate=gt, residual=r, config='deep64', in_bias=bi, in_act='silu' if pre else None)
    a = kernels.conv1x1_bias_act(x, w, b, 'silu', **kw)
    a2 = kernels.conv1x1_bias_act(x, w, b, 'silu', **kw)
    assert torch.equal(a, a2)
    with torch.inference_mode():
        out = torch.empty_like(a)
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.conv1x1_bias_act(x, w, b, 'silu', out=out, **kw)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                kernels.conv1x1_bias_act(x, w, b, 'silu', out=out, **kw)
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)


def _shifted(t, floats):
    big = torch.zeros(t.numel() + 8, device='cuda')
    v = big[floats:floats + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def test_shifted_aligned_base_is_accepted_and_unaligned_refused(hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W = 3, 100, 80, 2, 2
    x, w, b, gt, r, _ = _inputs(B, K, M, H, W, 9, True, True, False)
    ref = kernels.conv1x1_bias_act(x, w, b, 'relu', gate=gt, residual=r, config='tall')
    xs, ws, rs = _shifted(x, 4), _shifted(w, 4), _shifted(r, 4)    # 16 bytes past the allocation's base
    out = _shifted(torch.zeros_like(ref), 4)
    assert xs.data_ptr() % 16 == 0 and xs.data_ptr() % 32 != 0
    kernels.conv1x1_bias_act(xs, ws, b, 'relu', gate=gt, residual=rs, out=out, config='deep64')
    assert torch.equal(out, ref)
    null = ctypes.c_void_p(0)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    f = hip_lib.mtr_conv1x1_bias_act_pre
    args = lambda xx, ww, rr, yy: (p(xx), 0, p(ww), p(b), null, 0, p(gt), p(rr), 1, B, M, K, H * W, p(yy), null, 5)
    y = torch.full_like(ref, -7.0)
    for bad in (_shifted(x, 1), _shifted(x, 2)):                    # 4 and 8 bytes off
        assert f(*args(bad, w, r, y)) == -6                         # MTR_E_ALIGN
    assert f(*args(x, _shifted(w, 1), r, y)) == -6
    assert f(*args(x, _shifted(w, 2), r, y)) == -6
    assert f(*args(x, w, _shifted(r, 3), y)) == -6
    assert f(*args(x, w, r, _shifted(ref, 1))) == -6
    assert f(*args(x, w, r, _shifted(ref, 2))) == -6
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())


def test_refusals_of_the_pre_entry_under_code_5(hip_lib):
    """Every refusal in the order of the entry (NULL, dtype, shape, act codes, alignment, aliasing), nothing launched: y
    keeps its sentinels.  The _opts entry has no code 5; the plan is the same for a forced and an automatic choice."""
    from metrabs_amd import kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(1024, device='cuda')
    y = torch.full((1024,), -7.0, device='cuda')
    p, q = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(y.data_ptr())
    off = lambda base, n: ctypes.c_void_p(base.data_ptr() + n)
    f = hip_lib.mtr_conv1x1_bias_act_pre
    #  x, dtype, w, bias, in_bias, in_act, gate, residual, act, B, M, K, HW, y, stream, config
    assert f(null, 1, p, p, null, 0, null, null, 0, 1, 8, 8, 49, q, null, 5) == -1      # NULL first
    assert f(p, 0, null, p, null, 0, null, null, 0, 1, 8, 8, 16, q, null, 5) == -1
    assert f(p, 0, p, null, null, 0, null, null, 0, 1, 8, 8, 16, q, null, 5) == -1
    assert f(p, 0, p, p, null, 0, null, null, 0, 1, 8, 8, 16, null, null, 5) == -1
    assert f(p, 1, p, p, null, 0, null, null, 0, 1, 8, 8, 49, q, null, 5) == -3         # dtype before shape
    assert f(p, 0, p, p, null, 0, null, null, 7, 1, 8, 8, 49, q, null, 5) == -2         # shape before the act code
    assert f(p, 0, p, p, null, 0, null, null, 0, 1, 8, 6, 16, q, null, 5) == -2         # Cin = 6
    assert f(p, 0, p, p, null, 0, null, null, 0, -1, 8, 8, 16, q, null, 5) == -2
    assert f(p, 0, p, p, null, 0, null, null, 7, 1, 8, 8, 16, off(y, 4), null, 5) == -4  # act code before alignment
    assert f(p, 0, p, p, p, 7, null, null, 0, 1, 8, 8, 16, q, null, 5) == -4            # in_act code
    assert f(p, 0, p, p, null, 2, null, null, 0, 1, 8, 8, 16, q, null, 5) == -4         # in_act without in_bias
    assert f(p, 0, p, p, null, 0, null, null, 0, 1, 8, 8, 16, off(y, 4), null, 5) == -6
    assert f(p, 0, p, p, off(t, 2), 0, null, null, 0, 1, 8, 8, 16, q, null, 5) == -6    # in_bias: 4-byte aligned
    assert f(p, 0, p, p, null, 0, null, null, 0, 1, 8, 8, 16, p, null, 5) == -4         # y aliases x (behind alignment)
    assert f(p, 0, p, p, null, 0, null, p, 0, 1, 8, 8, 16, q, null, 5) == -4            # the skip aliases x
    assert f(p, 0, p, p, null, 0, null, null, 0, 0, 8, 8, 16, q, null, 5) == 0          # B = 0: nothing to do
    assert f(p, 0, p, p, null, 0, null, null, 0, 1, 8, 8, 16, q, null, 9) == -4         # no such configuration
    assert f(p, 0, p, p, null, 0, null, null, 0, 1, 8, 8, 16, q, null, 6) == -4
    g = hip_lib.mtr_conv1x1_bias_act_opts
    assert g(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, 5) == -4
    assert g(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, 4) == -4
    torch.cuda.synchronize()
    assert bool((y == -7.0).all())
    for M, K, HW, B in [(256, 1536, 64, 64), (8, 8, 4, 1), (160, 960, 256, 64), (48, 96, 4096, 64)]:
        assert kernels.conv1x1_plan(M, K, HW, B, 'deep64') == ('deep64', 2, 64, 64)
        auto = kernels.conv1x1_plan(M, K, HW, B)
        assert auto == kernels.conv1x1_plan(M, K, HW, B, 'auto')
        assert auto == kernels.conv1x1_plan(M, K, HW, B, auto[0])   # the automatic choice, forced, is itself


@pytest.fixture(scope='module')
def effnet():
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone('efficientnetv2-s').cuda(), 256, 'cuda', batch_size=4)
    return backbones.fold_batchnorm(net, fused_epilogue=True)


def test_network_gated_projects_run_on_k13(effnet):
    """Folded f32 EfficientNetV2-S at 256 px, batch 2: every gated project reports 'k13_gate' (k13_slower ended up empty:
    1536 -> 256 on 8x8 maps runs 'deep64'), no x * gate pass is left, the output is within 1e-4 relative (max-abs over
    max) of the same forward with K13 off, and the state dict keeps its keys."""
    from metrabs_amd import backbones, kernels
    fused = effnet
    keys = list(fused.state_dict())
    x = torch.rand(2, 3, 256, 256, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    muls = []
    orig_mul = torch.Tensor.__mul__

    def counting_mul(a, b):
        if isinstance(b, torch.Tensor) and b.dim() == 4 and b.shape[2:] == (1, 1) and a.dim() == 4 \
                and a.shape[2:] != (1, 1):
            muls.append(tuple(a.shape))
        return orig_mul(a, b)

    try:
        backbones.ConvBiasAct.use_k13 = False
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            a = fused(x)
        backbones.ConvBiasAct.use_k13 = True
        torch.Tensor.__mul__ = counting_mul
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            b = fused(x)
    finally:
        torch.Tensor.__mul__ = orig_mul
        backbones.ConvBiasAct.use_k13 = True
    assert float((a - b).abs().max()) <= 1e-4 * float(a.abs().max()), float((a - b).abs().max())
    slower = backbones.ConvBiasAct.k13_slower
    assert slower == frozenset()
    seen, n_library = {}, 0
    for blk in fused.modules():
        if not isinstance(blk, backbones.MBConv):
            continue
        layers = list(blk.block)
        for i, m in enumerate(layers):
            if i > 0 and isinstance(layers[i - 1], backbones.SqueezeExcite) and isinstance(m, backbones.ConvBNAct) \
                    and isinstance(m[0], backbones.ConvBiasAct):
                c = m[0].conv
                if m[0].last_path == 'library':
                    n_library += 1
                    continue
                assert m[0].last_path == 'k13_gate', (c.in_channels, c.out_channels, m[0].last_path)
                seen[(c.in_channels, c.out_channels)] = seen.get((c.in_channels, c.out_channels), 0) + 1
    assert n_library == 0 and len(muls) == n_library
    assert seen.get((1536, 256)) == 14 and seen.get((960, 256)) == 1
    assert kernels.conv1x1_plan(256, 1536, 64, 64) == ('deep64', 2, 64, 64)
    assert list(fused.state_dict()) == keys


def test_graphed_api_call_equals_eager(tmp_path, hip_lib):
    """A 256 px crop model with the folded f32 backbone (its stage-6 projects on 'deep64') through the drop-in API:
    graph-replayed batches return the eager call's bits."""
    import numpy as np
    from oracle import cases
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
    ests = {}
    for graphed in (False, True):
        est = loading.load_multiperson_model(d, fold_batchnorm=True, fused_epilogue=True)
        est.crop_model.deterministic_backbone = True
        est.graph_batches = graphed
        ests[graphed] = est
    images = torch.stack([cases.synth_images(1, 240, 320, 5 + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]

    def poses(est):
        with torch.inference_mode():
            r = est.estimate_poses_batched(images, boxes, num_aug=2)
        return torch.cat(r['poses3d']).clone()

    for _ in range(2):   # (the second call replays the graph)
        a, b = poses(ests[False]), poses(ests[True])
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())
    st = ests[True].graphs.stats
    assert st['captures'] >= 1 and st['replays'] >= 1, st
    paths = {(m.conv.in_channels, m.conv.out_channels): m.last_path
             for m in ests[True].crop_model.backbone.modules() if isinstance(m, backbones.ConvBiasAct)}
    assert paths[(1536, 256)] == 'k13_gate'
