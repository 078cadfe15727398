"""GPU: K10 (csrc/bias_act.hip: kernels.bias_act_, kernels.bias_act_rowmean_), the in-place bias + activation
(+ skip connection, + row mean) epilogue of the backbone's inference copy, against fp64, exactly on integers, call
against call and graph replay bit for bit, with guard bands around what it writes; and the folded + fused backbone
against the original network.  (K11, the depthwise 3x3 kernel with this epilogue, is in test_gpu_depthwise3x3.py;
its first 19 cases keep their ids here.)

The accuracy bound (no free tolerance), in the style of tests/test_gpu_depthwise5x5.py.  The input y is already of
the tensor's dtype T and the bias is f32, so the fp64 reference has the kernel's operands.  With u = 2^-24:
  * t = y + b is one f32 addition: |t_hat - t| <= u |t| <= u S with S = |y| + |b|;
  * the activation (common.h activate<>, K15's code) is Lipschitz with constant L <= 1.5 (hardswish: (2x + 3) / 6
    at x = 3; silu 1.1, relu and none 1), which carries that to 1.5 u S, and is itself evaluated in f32 with at most
    (8 + 2 |t|) u |act(t)| (hardswish: 5 roundings; silu: the rounded argument of exp2 costs 2 |t| u relative,
    v_exp_f32, the addition, v_rcp_f32 and the product 6 u more):   E = 1.5 u S + (8 + 2 |t|) u |act(t)|;
  * with a residual r (of dtype T, exact in f32) one more f32 addition, of a sum that is at most |act(t) + r| + E:
    E_r = E (1 + u) + u |act(t) + r|;
  * one rounding to T: u_out = 2^-24 (f32), 2^-11 (f16), 2^-8 (bf16), plus half the smallest f16 subnormal (2^-25):
  bound = E (1 + u_out) + u_out |ref| + tiny,   ref = act(t) (+ r)
  * the row mean is the f32 sum of the n = H * W STORED results (n - 1 additions in whatever order) times the
    rounded 1 / n: |mean_hat - mean(y)| <= (n + 1) u mean |y|.
Each test prints the largest observed error as a share of this bound.

Out of reach of a test: the WIDE instantiation of bias_act_kernel (64-bit index arithmetic) needs more than 2^32
vectors, 64 GiB of activations and up."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ACTS = [None, 'relu', 'silu', 'hardswish']
U = 2.0 ** -24
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float32: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -126}
VEC = {torch.float32: 4, torch.float16: 8, torch.bfloat16: 8}   # elements of a 16-byte vector


def _act64(v, act):
    if act == 'relu':
        return v.clamp_min(0)
    if act == 'silu':
        return v * torch.sigmoid(v)
    if act == 'hardswish':
        return v * (v + 3).clamp(0, 6) / 6
    return v


def _inputs(shape, dtype, seed, residual=False):
    g = torch.Generator(device='cuda').manual_seed(seed)
    y = (torch.randn(shape, device='cuda', generator=g) * 3).to(dtype)   # of the tensor dtype: the kernel's operand
    b = torch.randn(shape[1], device='cuda', generator=g)
    r = (torch.randn(shape, device='cuda', generator=g) * 2).to(dtype) if residual else None
    return y, b, r


def _ref_and_bound(y, b, r, act):
    """(fp64 result, the bound of the module docstring) of the input y (of the tensor's dtype), bias and skip."""
    uo, tiny = U_OUT[y.dtype], TINY[y.dtype]
    yd, bd = y.double(), b.double().view(1, -1, 1, 1)
    t = yd + bd
    ref = _act64(t, act)
    E = 1.5 * U * (yd.abs() + bd.abs()) + (8 + 2 * t.abs()) * U * ref.abs()
    if r is not None:
        ref = ref + r.double()
        E = E * (1 + U) + U * ref.abs()
    return ref, E * (1 + uo) + uo * ref.abs() + tiny


def _check(y, b, r, act, got, mean=None, tag=''):
    """got (and the row mean of got) against the fp64 bound, in slices of the batch of at most 2^22 elements.
    Returns (largest share of the bound, largest share of the mean's bound)."""
    assert got.shape == y.shape and got.dtype == y.dtype
    uo, tiny = U_OUT[y.dtype], TINY[y.dtype]
    B = y.shape[0]
    step = max(1, (1 << 22) // max(1, y[0].numel()))
    share = mshare = 0.0
    for i in range(0, B, step):
        ref, bound = _ref_and_bound(y[i:i + step], b, None if r is None else r[i:i + step], act)
        gd = got[i:i + step].double()
        share = max(share, float(((gd - ref).abs() / bound).max()))
        if mean is not None:
            hw = y.shape[2] * y.shape[3]
            mbound = (hw + 1) * U * gd.abs().mean((2, 3)) + 2.0 ** -126
            assert mean.shape == y.shape[:2] and mean.dtype == torch.float32
            mshare = max(mshare, float(((mean[i:i + step].double() - gd.mean((2, 3))).abs() / mbound).max()))
    assert share <= 1.0 and mshare <= 1.0, (tag, share, mshare)
    return share, mshare


# (64, 24, 128, 128) is past the cap of 8,192 workgroups: the grid-stride loop.  C in {1, 7, 130, 1536} and
# H * W in {8, 16, 56, 784, 16384} (/ 4 or / 8 elements per vector) are the divisors of the two fastdivs.
BIAS_ACT_SHAPES = [(3, 5, 8, 8), (2, 1536, 8, 8), (64, 24, 128, 128), (1, 7, 2, 4), (5, 960, 16, 16),
                   (3, 1, 2, 4), (2, 1536, 4, 4), (2, 130, 7, 8), (2, 7, 28, 28), (1, 130, 128, 128), (2, 1, 128, 128),
                   (3, 1536, 2, 4)]


def test_the_bias_act_shapes_reach_the_grid_stride_loop_and_the_divisors():
    for dtype in DTYPES:
        n_vec = [s[0] * s[1] * s[2] * s[3] // VEC[dtype] for s in BIAS_ACT_SHAPES]
        assert all(s[2] * s[3] % VEC[dtype] == 0 for s in BIAS_ACT_SHAPES)
        assert max((n + 255) // 256 for n in n_vec) > 256 * 32          # more vectors than lanes in the grid
        assert any(n % 256 for n in n_vec) and min(n_vec) < 64          # a ragged last workgroup, less than a wave
    assert {s[1] for s in BIAS_ACT_SHAPES} >= {1, 7, 130, 1536}
    assert {s[2] * s[3] for s in BIAS_ACT_SHAPES} >= {8, 16, 56, 784, 16384}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', BIAS_ACT_SHAPES)
@pytest.mark.parametrize('act', ACTS)
def test_bias_act_vs_torch(shape, act, dtype, hip_lib):
    """Without and with the skip connection, against fp64 under the bound above.  (The name, kept with the test's
    ids, is from when the reference was torch's own f32 ops under a free tolerance.)"""
    from metrabs_amd import kernels
    for residual in (False, True):
        y, b, r = _inputs(shape, dtype, sum(shape), residual)
        work = y.clone()
        r0 = None if r is None else r.clone()
        got = kernels.bias_act_(work, b, act, residual=r)
        assert got.data_ptr() == work.data_ptr()   # in place
        assert r is None or torch.equal(r, r0)
        share, _ = _check(y, b, r, act, got, tag=shape)
        print(f'[k10] bias_act {shape} {str(dtype)[6:]} act={act} residual={residual}: largest share of the bound '
              f'{share:.3f}')


# rows of H * W / VEC vectors: up to 16 vectors a row has 16 lanes (LPR), above that 64
ROWMEAN_SHAPES = [(3, 5, 8, 8), (2, 1536, 8, 8), (64, 960, 16, 16), (1, 7, 2, 4), (2, 9, 28, 28), (130, 3, 4, 4),
                  (1, 1, 8, 8), (1, 9, 28, 28), (2, 5, 8, 16), (2, 5, 8, 17), (1, 1, 8, 17)]
ROWMEAN_F32_ONLY = [(2, 5, 4, 17)]   # H * W = 68: 17 f32 vectors, no whole number of 16-bit ones


def _rowmean_shapes(dtype):
    return ROWMEAN_SHAPES + (ROWMEAN_F32_ONLY if dtype == torch.float32 else [])


def test_the_rowmean_shapes_sit_on_both_sides_of_the_lane_switch():
    for dtype in DTYPES:
        shapes = _rowmean_shapes(dtype)
        assert all(s[2] * s[3] % VEC[dtype] == 0 for s in shapes)
        hw_vec = {s[2] * s[3] // VEC[dtype] for s in shapes}
        assert {16, 17} <= hw_vec and min(hw_vec) < 16                      # at the switch, right above it, below
        assert any(v > 64 and v % 64 for v in hw_vec)                       # 28x28: no multiple of the 64 lanes
        for lpr_16 in (True, False):   # 4 rows or 1 row per wave, 4 waves per workgroup: a last one with idle lanes
            rows = {s[0] * s[1] for s in shapes if (s[2] * s[3] // VEC[dtype] <= 16) == lpr_16}
            assert any(n % 4 for n in rows), rows
        assert {s[0] * s[1] for s in shapes} >= {1, 9, 390}


def _rowmean_case(shape, dtype):
    """Every activation: the same result tensor as bias_act_, bit for bit, and the mean over H*W of that result."""
    from metrabs_amd import kernels
    for act in ACTS:
        y, b, _ = _inputs(shape, dtype, sum(shape) + 1)
        plain = kernels.bias_act_(y.clone(), b, act)
        work = y.clone()
        got, mean = kernels.bias_act_rowmean_(work, b, act)
        assert got.data_ptr() == work.data_ptr() and torch.equal(got, plain)
        share, mshare = _check(y, b, None, act, got, mean, tag=shape)
        print(f'[k10] rowmean {shape} {str(dtype)[6:]} act={act}: largest share of the bound {share:.3f}, of the '
              f'mean\'s summation bound {mshare:.3f}')


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', ROWMEAN_SHAPES)
def test_bias_act_rowmean_vs_torch(shape, dtype, hip_lib):
    """(The name, kept with the test's ids, is from when the reference was torch's f32 mean under a free tolerance.)"""
    _rowmean_case(shape, dtype)


@pytest.mark.parametrize('shape', ROWMEAN_F32_ONLY)
def test_bias_act_rowmean_right_above_the_lane_switch_in_f32(shape, hip_lib):
    _rowmean_case(shape, torch.float32)


# ---- K11 under the ids its first 19 cases have always had

@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('cfg', [(2, 960, 16, 16, 1, 1), (3, 256, 32, 32, 2, 1), (2, 96, 18, 18, 2, 0),
                                 (5, 1536, 8, 8, 1, 1), (1, 7, 4, 8, 1, 1), (2, 5, 9, 9, 2, 0), (70, 3, 16, 16, 1, 1),
                                 (3, 4, 32, 32, 1, 1), (2, 5, 64, 64, 2, 1), (2, 6, 10, 18, 1, 0),
                                 (64, 960, 16, 16, 1, 1), (33, 130, 8, 8, 1, 1), (2, 3, 24, 40, 1, 1)])
def test_depthwise3x3_bias_act_vs_torch(cfg, dtype, hip_lib):
    """K11's tests are in test_gpu_depthwise3x3.py, where these 13 cases run for every activation and dtype (EARLIER in
    its case list).  They stay here too, under the ids they have had since K11 went in and on that file's fp64
    reference and bound in place of torch's f32 convolution and a free tolerance: SiLU with the mean, the call
    without the mean (same bits), and no activation."""
    import test_gpu_depthwise3x3 as k11
    from metrabs_amd import kernels
    B, C, H, W, stride, pad = cfg
    assert cfg in [c[:6] for c in k11.EARLIER]
    x, w, b = k11._inputs(B, C, H, W, dtype, sum(cfg))
    got, mean = kernels.depthwise3x3_bias_act(x, w, b, 'silu', stride, pad, want_mean=True)
    k11._check(x, w, b, 'silu', stride, pad, [(got, mean)], tag=cfg)
    assert torch.equal(kernels.depthwise3x3_bias_act(x, w, b, 'silu', stride, pad), got)
    none = kernels.depthwise3x3_bias_act(x, w, b, None, stride, pad)
    k11._check(x, w, b, None, stride, pad, [(none, None)], tag=cfg)


@pytest.mark.parametrize('dtype', [torch.float32, torch.float16])
@pytest.mark.parametrize('cfg', [(3, 960, 16, 16, 2, (0, 2, 0, 2)), (2, 256, 32, 32, 2, (0, 1, 0, 1)),
                                 (2, 7, 8, 24, 2, (1, 0, 1, 0)), (2, 5, 16, 16, 1, (1, 1, 1, 1)),
                                 (2, 6, 14, 12, 1, (0, 2, 1, 1)), (70, 3, 16, 16, 2, (0, 2, 0, 2))])
def test_depthwise3x3_with_folded_zero_padding(cfg, dtype, hip_lib):
    """The explicit ZeroPad2d of the reference's TF-'SAME' stride-2 layers as an argument of K11; as above, these six
    cases also run in test_gpu_depthwise3x3.py and keep their ids here, on the fp64 reference of the padded input."""
    import test_gpu_depthwise3x3 as k11
    from metrabs_amd import kernels
    B, C, H, W, stride, pads = cfg
    assert cfg in [c[:6] for c in k11.EARLIER]
    x, w, b = k11._inputs(B, C, H, W, dtype, sum(cfg[:5]) + sum(pads))
    got, mean = kernels.depthwise3x3_bias_act(x, w, b, 'silu', stride, pads, want_mean=True)
    k11._check(x, w, b, 'silu', stride, pads, [(got, mean)], tag=cfg)


# ---- exactly on integers

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', [None, 'relu'])
def test_exact_on_integers(act, dtype, hip_lib):
    """Integer y in -8 .. 8, bias in -C/2 .. C/2, residual in -4 .. 4: every sum is an integer of at most 16, exact in
    all three dtypes."""
    from metrabs_amd import kernels
    for shape in [(3, 5, 8, 8), (2, 9, 4, 17 if dtype == torch.float32 else 18), (1, 7, 28, 28)]:
        g = torch.Generator().manual_seed(sum(shape))
        y = torch.randint(-8, 9, shape, generator=g).double()
        b = (torch.arange(shape[1]) - shape[1] // 2).double()
        r = torch.randint(-4, 5, shape, generator=g).double()
        want = _act64(y + b.view(1, -1, 1, 1), act)
        assert float(want.abs().max()) >= 8 and float((want + r).abs().max()) <= 16
        yc, bc, rc = y.cuda().to(dtype), b.cuda().float(), r.cuda().to(dtype)
        assert torch.equal(kernels.bias_act_(yc.clone(), bc, act).double().cpu(), want)
        assert torch.equal(kernels.bias_act_(yc.clone(), bc, act, residual=rc).double().cpu(), want + r)
        got, mean = kernels.bias_act_rowmean_(yc.clone(), bc, act)
        assert torch.equal(got.double().cpu(), want)
        # an exact integer sum times the rounded 1 / n: two roundings
        mwant = want.mean((2, 3))
        assert bool(((mean.double().cpu() - mwant).abs() <= (2 * U + U * U) * mwant.abs()).all())


# ---- the kernels write what they own and nothing else

_PATTERN = {4: (torch.int32, 0x5A5A5A5A), 2: (torch.int16, 0x5A5A)}


def _banded(n, dtype, band=256):
    """(whole, interior): n elements of dtype at a 16-byte-aligned offset inside a buffer prefilled with a fixed bit
    pattern, `band` elements of it on each side; `whole` is the integer view everything is compared through."""
    itype, pattern = _PATTERN[torch.empty(0, dtype=dtype).element_size()]
    whole = torch.full((n + 2 * band,), pattern, device='cuda', dtype=itype)
    inner = whole[band:band + n].view(dtype)
    assert inner.data_ptr() % 16 == 0
    return whole, inner


def _bands_untouched(whole, n, band=256):
    pattern = _PATTERN[whole.element_size()][1]
    return bool((whole[:band] == pattern).all()) and bool((whole[band + n:] == pattern).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(3, 5, 8, 8), (1, 7, 2, 4), (1, 9, 28, 28), (130, 3, 4, 4), (1, 1, 8, 24)])
def test_guard_bands_around_activations_residual_and_means(shape, dtype, hip_lib):
    """Through the C entries, on buffers with a fixed bit pattern on both sides: idle lanes recompute the last row and
    must not store it; the residual is read only."""
    from metrabs_amd import _lib, kernels
    B, C, H, W = shape
    n = B * C * H * W
    src, b, r = _inputs(shape, dtype, sum(shape) + 2, residual=True)
    want = kernels.bias_act_(src.clone(), b, 'silu', residual=r)
    want_plain, want_mean = kernels.bias_act_rowmean_(src.clone(), b, 'silu')
    stream, code, silu = _lib.current_stream_ptr(src.device), _lib.dtype_code(dtype), kernels.ACT_CODES['silu']
    ywhole, y = _banded(n, dtype)
    rwhole, res = _banded(n, dtype)
    y.copy_(src.view(-1))
    res.copy_(r.view(-1))
    before = rwhole.clone()
    assert hip_lib.mtr_bias_act_nchw(y.data_ptr(), code, b.data_ptr(), res.data_ptr(), silu, B, C, H * W, stream) == 0
    torch.cuda.synchronize()
    assert _bands_untouched(ywhole, n) and torch.equal(rwhole, before)
    assert torch.equal(y.view(shape), want)
    ywhole, y = _banded(n, dtype)
    mwhole, mean = _banded(B * C, torch.float32)
    y.copy_(src.view(-1))
    assert hip_lib.mtr_bias_act_rowmean_nchw(y.data_ptr(), code, b.data_ptr(), silu, B, C, H * W, mean.data_ptr(),
                                             stream) == 0
    torch.cuda.synchronize()
    assert _bands_untouched(ywhole, n) and _bands_untouched(mwhole, B * C)
    assert torch.equal(y.view(shape), want_plain) and torch.equal(mean.view(B, C), want_mean)


# ---- what the entries refuse

def test_bias_act_rejects_what_it_cannot_vectorise(hip_lib):
    from metrabs_amd import kernels
    y = torch.zeros(2, 3, 3, 3, device='cuda')  # H*W = 9: a 16-byte vector would straddle channels
    with pytest.raises(RuntimeError):
        kernels.bias_act_(y, torch.zeros(3, device='cuda'), 'silu')
    with pytest.raises(ValueError):
        kernels.bias_act_(torch.zeros(2, 4, 4, 4, device='cuda').permute(0, 2, 3, 1), torch.zeros(4, device='cuda'), None)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_base_that_is_not_16_byte_aligned_is_refused(dtype, hip_lib):
    """MTR_E_ALIGN (-6) instead of running on misaligned vectors; nothing is written."""
    from metrabs_amd import _lib, kernels
    shape = (2, 5, 8, 8)
    src, b, r = _inputs(shape, dtype, 3, residual=True)
    buf = torch.zeros(src.numel() + 8, device='cuda', dtype=dtype)
    y = buf[1:1 + src.numel()].view(shape)
    y.copy_(src)
    assert y.is_contiguous() and y.data_ptr() % 16 != 0
    rbuf = torch.zeros(src.numel() + 8, device='cuda', dtype=dtype)
    rs = rbuf[1:1 + src.numel()].view(shape)
    rs.copy_(r)
    with pytest.raises(RuntimeError, match='code -6'):
        kernels.bias_act_(y, b, 'relu')
    with pytest.raises(RuntimeError, match='code -6'):
        kernels.bias_act_(src.clone(), b, 'relu', residual=rs)
    with pytest.raises(RuntimeError, match='code -6'):
        kernels.bias_act_rowmean_(y, b, 'relu')
    stream, code = _lib.current_stream_ptr(src.device), _lib.dtype_code(dtype)
    assert hip_lib.mtr_bias_act_nchw(y.data_ptr(), code, b.data_ptr(), None, 1, 2, 5, 64, stream) == -6
    mean = torch.zeros(2, 5, device='cuda')
    assert hip_lib.mtr_bias_act_rowmean_nchw(y.data_ptr(), code, b.data_ptr(), 1, 2, 5, 64, mean.data_ptr(), stream) == -6
    torch.cuda.synchronize()
    assert torch.equal(y, src) and not mean.any()


# ---- call against call, graph replay

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape,act', [((3, 5, 8, 8), 'silu'), ((2, 9, 28, 28), 'hardswish'), ((5, 960, 16, 16), 'relu')])
def test_call_against_call_and_graph_replay(shape, act, dtype, hip_lib):
    from metrabs_amd import kernels
    src, b, r = _inputs(shape, dtype, sum(shape) + 5, residual=True)
    a = kernels.bias_act_(src.clone(), b, act, residual=r)
    assert torch.equal(a, kernels.bias_act_(src.clone(), b, act, residual=r))
    m, mean = kernels.bias_act_rowmean_(src.clone(), b, act)
    m2, mean2 = kernels.bias_act_rowmean_(src.clone(), b, act)
    assert torch.equal(m, m2) and torch.equal(mean, mean2)
    with torch.inference_mode():
        ga, gm = src.clone(), src.clone()
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.bias_act_(src.clone(), b, act, residual=r)
            kernels.bias_act_rowmean_(src.clone(), b, act)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                kernels.bias_act_(ga, b, act, residual=r)
                _, gmean = kernels.bias_act_rowmean_(gm, b, act)
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(2):
            ga.copy_(src)    # the kernels work in place: the graph's buffers get their inputs back
            gm.copy_(src)
            gmean.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(ga, a) and torch.equal(gm, m) and torch.equal(gmean, mean)


# ---- inside the network

@pytest.mark.parametrize('name,res', [('effnetv2-s', 256), ('mobilenetv3', 256), ('resnet18', 256),
                                      ('effnetv2-s', 224), ('effnetv2-s', 160), ('mobilenetv3', 224)])
def test_folded_fused_backbone_is_the_same_function(name, res, hip_lib):
    """(224 / 160 px: 7x7 = 49 and 5x5 = 25-position maps are not a multiple of K10's 16-byte vectors:
    those layers must take the torch ops, not raise.)"""
    from metrabs_amd import backbones
    torch.manual_seed(0)
    net = backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=4)
    fused = backbones.fold_batchnorm(net, fused_epilogue=True)
    assert any(isinstance(m, backbones.DepthwiseBiasAct) for m in fused.modules()) == (name != 'resnet18')
    n_se = sum(isinstance(m, backbones.SqueezeExcite) for m in fused.modules())
    assert sum(bool(m.mean_from) for m in fused.modules() if isinstance(m, backbones.SqueezeExcite)) == n_se
    x = torch.rand(4, 3, res, res, device='cuda')
    with torch.inference_mode():
        a, b = net(x), fused(x)
        with torch.autocast('cuda', dtype=torch.float16):
            c = fused(x)
    assert float((a - b).abs().max()) <= 1e-3 * float(a.abs().max())
    assert c.dtype == torch.float16 and float((a - c.float()).abs().max()) <= 0.1 * float(a.abs().max())
