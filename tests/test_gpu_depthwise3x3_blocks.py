"""GPU: K18 (csrc/depthwise3x3_blocks.hip, kernels.depthwise3x3_blocks_bias_act) -- the stride-1, padding-1 depthwise
3x3 + bias + activation (+ the plane mean) on register blocks -- against fp64, bit for bit against K11's generic
kernel, block shape against block shape, exactly on integers, call against call and graph replay, with guard bands
around what it writes, every refusal, and inside fold_batchnorm(block_depthwise=True), the loaders and the API.

The accuracy bound is K11's (tests/test_gpu_depthwise3x3.py), restated; nothing here is looser.  Inputs are rounded
to the tensor's dtype first, weights and bias are f32, so every product x*w the kernel forms has the fp64 reference's
operands.  With u = 2^-24:
  * pre-activation v: nine fma from 0 and the bias last (10 f32 roundings); every partial sum is at most
    S = sum |x*w| + |b| in magnitude: |v_hat - v| <= gamma_10 S < 11 u S;
  * the activation (common.h activate<>) is Lipschitz with constant L <= 1.5 (hardswish; silu 1.1, relu and none 1),
    which carries that error to 1.5 * 11 u S, and is itself evaluated in f32: hardswish an addition, a clamp, two
    products and the rounded constant 1/6; silu x * rcp(1 + exp2(-x log2 e)): together at most
    (8 + 2 |v|) u |act(v)|;
  * one rounding to the output dtype: u_out |y_hat| with u_out = 2^-24 (f32), 2^-11 (f16), 2^-8 (bf16), plus half the
    smallest subnormal for f16 (2^-25).
  bound = E (1 + u_out) + u_out |act(v)| + tiny,   E = 1.5 * 11 u S + (8 + 2 |v|) u |act(v)|
  * the mean is the f32 sum of the n = H * W STORED outputs times the rounded 1 / n:
    |mean_hat - mean(y)| <= (n + 1) u mean |y|.
Each test prints the largest observed error as a share of this bound.

The bit contract: y and the mean are torch.equal to kernels.depthwise3x3_bias_act on the same tensors wherever that
call reaches K11's generic kernel.  On the three shapes K11's block kernel would take (4x4, 8x8, 16x16) K11 is called
on a base shifted by one element, which tests/test_gpu_depthwise3x3.py proves to reach the generic kernel.

The C entry has neither a stride nor a padding argument; those refusals are the query's, and a layer with them never
asks for K18 (the network tests assert the stride-2 and padded layers' paths)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
DTYPES = [F32, F16, BF16]
ACTS = [None, 'relu', 'silu', 'hardswish']
U = 2.0 ** -24
U_OUT = {F32: 2.0 ** -24, F16: 2.0 ** -11, BF16: 2.0 ** -8}
TINY = {F32: 2.0 ** -126, F16: 2.0 ** -25, BF16: 2.0 ** -126}

# (B, C, H, W): what each is there for
SMALL = [
    (2, 3, 12, 12),      # 3 blocks per row padded to 4 lanes
    (3, 3, 6, 8), (2, 3, 10, 16),   # H % 4 != 0: a partial block row
    (2, 3, 20, 28),      # 7 padded to 8 lanes
    (2, 3, 24, 40), (1, 5, 28, 44), (1, 5, 32, 48),   # 10, 11, 12 padded to 16 lanes; several chunks of the mean
    (1, 5, 28, 64),      # a plane row is exactly one DPP row
    (1, 3, 64, 64),      # a power-of-two plane K11's block kernel refuses; one workgroup per plane
    (1, 3, 8, 72), (1, 3, 12, 128), (1, 2, 128, 128),   # rows cut into 16-lane segments, planes walked in passes
    (2, 3, 4, 4), (2, 3, 8, 8), (2, 3, 16, 16),   # one-lane and small planes, several planes per wave
    (70, 3, 12, 12), (4099, 5, 12, 12),   # ragged last workgroups, planes that straddle waves
]
# the layer classes of EfficientNetV2-L at 384 px and MobileNetV3 at 256 px
REAL = [(2, 768, 24, 24), (2, 1344, 24, 24), (2, 2304, 12, 12), (2, 3840, 12, 12), (2, 16, 128, 128),
        (2, 72, 64, 64)]
REAL_ACT = {F32: 'silu', F16: 'hardswish', BF16: 'relu'}


@pytest.fixture(autouse=True)
def _leave_the_device_idle():
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


def test_the_case_list_is_what_it_says():
    from metrabs_amd import kernels
    eligible = [s for s in SMALL if kernels.k11_takes_block_kernel(s[2], s[3])]
    assert eligible == [(2, 3, 4, 4), (2, 3, 8, 8), (2, 3, 16, 16)]
    assert not any(kernels.k11_takes_block_kernel(s[2], s[3]) for s in REAL)
    for B, C, H, W in SMALL + REAL:
        assert kernels.depthwise3x3_blocks_supported(F32, H, W)
    assert any(H % 4 for _, _, H, _ in SMALL) and any(W > 64 for *_, W in SMALL)


# ---- reference and bound

def _act64(v, act):
    if act == 'relu':
        return v.clamp_min(0)
    if act == 'silu':
        return v * torch.sigmoid(v)
    if act == 'hardswish':
        return v * (v + 3).clamp(0, 6) / 6
    return v


def _inputs(B, C, H, W, dtype, seed, device='cuda'):
    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(B, C, H, W, device=device, generator=g).to(dtype)   # rounded to the tensor dtype first
    w = torch.randn(C, 1, 3, 3, device=device, generator=g) * 0.4
    b = torch.randn(C, device=device, generator=g)
    return x, w, b


def _conv64(x, w, b):
    """fp64: (v, S), v = the stride-1 padding-1 convolution plus bias as nine shifted slices of the padded input
    times w[c, ky, kx], S = the same on absolute values."""
    xd = F.pad(x.double(), (1, 1, 1, 1))
    B, C, H, W = x.shape
    wd, bd = w.double().reshape(C, 9), b.double().view(1, C, 1, 1)
    v = bd.expand(B, C, H, W).clone()
    S = bd.abs().expand(B, C, H, W).clone()
    xa = xd.abs()
    for ky in range(3):
        for kx in range(3):
            wk = wd[:, 3 * ky + kx].view(1, C, 1, 1)
            v.addcmul_(xd[:, :, ky:ky + H, kx:kx + W], wk)
            S.addcmul_(xa[:, :, ky:ky + H, kx:kx + W], wk.abs())
    return v, S


def test_the_reference_is_the_grouped_convolution():
    for H, W in [(5, 8), (12, 12)]:
        x, w, b = _inputs(2, 3, H, W, F32, 11 * H + W, device='cpu')
        v, S = _conv64(x, w, b)
        want = F.conv2d(x.double(), w.double(), b.double(), 1, 1, groups=3)
        assert bool(((v - want).abs() <= 22 * 2.0 ** -53 * S).all())


@functools.lru_cache(maxsize=None)
def _conv_case(B, C, H, W, dtype, seed):
    """Inputs and the fp64 pre-activation (v, S) of one case: computed once, shared by the activations, never
    modified."""
    x, w, b = _inputs(B, C, H, W, dtype, seed)
    return (x, w, b) + _conv64(x, w, b)


def _bound(v, S, dtype, act):
    """(fp64 result, the bound of the module docstring) from _conv64's (v, S)."""
    ref = _act64(v, act)
    uo = U_OUT[dtype]
    E = 1.5 * 11 * U * S + (8 + 2 * v.abs()) * U * ref.abs()
    return ref, E * (1 + uo) + uo * ref.abs() + TINY[dtype]


def _ref_and_bound(x, w, b, act):
    """(fp64 result, bound) of any tensors: what _check is given (tests/conv_fuzz.py)."""
    return _bound(*_conv64(x, w, b), x.dtype, act)


def _case(B, C, H, W, dtype, act, seed):
    x, w, b, v, S = _conv_case(B, C, H, W, dtype, seed)
    return (x, w, b) + _bound(v, S, dtype, act)


def _check(ref, bound, y, mean, tag):
    """(share of the bound, share of the mean's bound) of one result; asserts both are at most 1."""
    assert y.shape == ref.shape
    yd = y.double()
    share = float(((yd - ref).abs() / bound).max())
    mshare = 0.0
    if mean is not None:
        hw = y.shape[2] * y.shape[3]
        mbound = (hw + 1) * U * yd.abs().mean((2, 3)) + 2.0 ** -126
        assert mean.shape == y.shape[:2] and mean.dtype == F32
        mshare = float(((mean.double() - yd.mean((2, 3))).abs() / mbound).max())
    assert share <= 1.0 and mshare <= 1.0, (tag, share, mshare)
    return share, mshare


def _shifted(x):
    """The same tensor at a base one element further: not 16-byte aligned, K11's generic kernel (scalar rows)."""
    buf = torch.zeros(x.numel() + 8, device=x.device, dtype=x.dtype)
    s = buf[1:1 + x.numel()].view_as(x)
    s.copy_(x)
    assert s.is_contiguous() and s.data_ptr() % 16 != 0
    return s


def _one_case(kernels, shape, dtype, act, seed):
    """Everything that is checked on each case.  -> the two shares."""
    B, C, H, W = shape
    x, w, b, ref, bound = _case(B, C, H, W, dtype, act, seed)
    assert x.data_ptr() % 16 == 0
    x0 = x.clone()
    y, mean = kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True)
    assert y.dtype == dtype and y.is_contiguous()
    assert torch.equal(y, kernels.depthwise3x3_blocks_bias_act(x, w, b, act)), shape   # without the mean
    share, mshare = _check(ref, bound, y, mean, (shape, dtype, act))
    # K11's generic kernel, bit for bit
    xk = _shifted(x) if kernels.k11_takes_block_kernel(H, W) else x
    ky, kmean = kernels.depthwise3x3_bias_act(xk, w, b, act, 1, 1, want_mean=True)
    assert torch.equal(y, ky), (shape, dtype, act, float((y.double() - ky.double()).abs().max()))
    assert torch.equal(mean, kmean), (shape, dtype, act, float((mean - kmean).abs().max()))
    # both block shapes
    y4, m4 = kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True, block_cols=4)
    assert torch.equal(y4, y) and torch.equal(m4, mean), shape
    if dtype != F32 and W % 8 == 0:
        y8, m8 = kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True, block_cols=8)
        assert torch.equal(y8, y) and torch.equal(m8, mean), shape
    assert torch.equal(x, x0)   # x untouched
    return share, mshare


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
def test_small_shapes_match_fp64_and_k11s_generic_kernel(act, dtype, hip_lib):
    from metrabs_amd import kernels
    worst, mworst, where = 0.0, 0.0, None
    for i, shape in enumerate(SMALL):
        share, mshare = _one_case(kernels, shape, dtype, act, 3000 + i)
        if share > worst:
            worst, where = share, shape
        mworst = max(mworst, mshare)
    print(f'[k18] small {str(dtype)[6:]} act={act}: largest share of the bound {worst:.3f} at {where}, of the '
          f'mean\'s summation bound {mworst:.3f}')


@pytest.mark.parametrize('dtype', DTYPES)
def test_real_layer_classes_match_fp64_and_k11s_generic_kernel(dtype, hip_lib):
    from metrabs_amd import kernels
    worst, mworst, where = 0.0, 0.0, None
    for i, shape in enumerate(REAL):
        share, mshare = _one_case(kernels, shape, dtype, REAL_ACT[dtype], 4000 + i)
        if share > worst:
            worst, where = share, shape
        mworst = max(mworst, mshare)
    print(f'[k18] real {str(dtype)[6:]} act={REAL_ACT[dtype]}: largest share of the bound {worst:.3f} at {where}, '
          f'of the mean\'s summation bound {mworst:.3f}')


# ---- exactly on integers, and a constant plane

_TAPS = (3.0 * (torch.arange(9, dtype=torch.float32) - 4.0)).view(1, 1, 3, 3)   # different at every tap, asymmetric
_EXACT_SHAPES = [(4, 4), (12, 12), (10, 16), (20, 28), (24, 40), (8, 72), (7, 128), (64, 64)]


def _exact_case(B, C, H, W, seed):
    """Integers in -1 .. 1 inside the plane and in -2 .. 2 on its border rows and columns, taps -12 .. 12 in steps of
    3 with the sign flipped on every other channel, an integer bias: every product, partial sum and output is a
    small integer, exact in f32 and -- at most 256, asserted -- in bf16."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-1, 2, (B, C, H, W), generator=g).float()
    edge = torch.randint(-2, 3, (B, C, H, W), generator=g).float()
    border = torch.zeros(H, W, dtype=torch.bool)
    border[0], border[-1], border[:, 0], border[:, -1] = True, True, True, True
    x = torch.where(border, edge, x)
    w = _TAPS.repeat(C, 1, 1, 1) * torch.tensor([1.0, -1.0]).repeat((C + 1) // 2)[:C].view(C, 1, 1, 1)
    b = torch.arange(C, dtype=torch.float32) - C // 2
    return x, w, b


@pytest.mark.parametrize('dtype', DTYPES)
def test_exact_on_integers(dtype, hip_lib):
    from metrabs_amd import kernels
    for H, W in _EXACT_SHAPES:
        x, w, b = _exact_case(3, 6, H, W, 7 * H + W)
        want = F.conv2d(x.double(), w.double(), b.double(), 1, 1, groups=6)
        assert 32 <= float(want.abs().max()) <= 256 and torch.equal(want, want.round())
        for bc in (4, 8) if dtype != F32 and W % 8 == 0 else (4,):
            y, mean = kernels.depthwise3x3_blocks_bias_act(x.cuda().to(dtype), w.cuda(), b.cuda(), None,
                                                           want_mean=True, block_cols=bc)
            assert torch.equal(y.double().cpu(), want), (H, W, bc, float((y.double().cpu() - want).abs().max()))
            mwant = want.mean((2, 3))
            assert bool(((mean.double().cpu() - mwant).abs() <= (2 * U + U * U) * mwant.abs()).all()), (H, W)


@pytest.mark.parametrize('dtype', DTYPES)
def test_a_constant_plane_counts_its_taps(dtype, hip_lib):
    """x = 1, every tap 1, no bias: an output is the number of its taps inside the plane -- 9, 6 on an edge, 4 in a
    corner (fewer on planes one or two rows high).  A halo taken from the neighbouring plane row, plane or block
    would give a border output one of the interior's values."""
    from metrabs_amd import kernels
    for H, W in [(4, 4), (1, 8), (2, 12), (12, 12), (10, 16), (24, 24), (9, 72), (128, 128), (64, 64)]:
        x = torch.ones(3, 2, H, W, device='cuda', dtype=dtype)
        w, b = torch.ones(2, 1, 3, 3, device='cuda'), torch.zeros(2, device='cuda')
        rows = torch.tensor([min(i + 1, H - 1) - max(i - 1, 0) + 1 for i in range(H)], dtype=torch.float64)
        cols = torch.tensor([min(j + 1, W - 1) - max(j - 1, 0) + 1 for j in range(W)], dtype=torch.float64)
        want = (rows[:, None] * cols[None, :]).expand(3, 2, H, W)
        for bc in (4, 8) if dtype != F32 and W % 8 == 0 else (4,):
            y, mean = kernels.depthwise3x3_blocks_bias_act(x, w, b, None, want_mean=True, block_cols=bc)
            assert torch.equal(y.double().cpu(), want), (H, W, bc)
            mwant = want.mean((2, 3))
            assert bool(((mean.double().cpu() - mwant).abs() <= (2 * U + U * U) * mwant).all()), (H, W)


# ---- call against call, graph replay

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,C,H,W,act', [(70, 3, 12, 12, 'silu'), (2, 5, 24, 40, 'hardswish'), (1, 2, 128, 128, 'relu'),
                                         (3, 3, 6, 8, None)])
def test_call_against_call_and_graph_replay(B, C, H, W, act, dtype, hip_lib):
    from metrabs_amd import kernels
    x, w, b = _inputs(B, C, H, W, dtype, 500 + C)
    y, mean = kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True)
    y3, mean3 = kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True)
    assert torch.equal(y, y3) and torch.equal(mean, mean3)
    with torch.inference_mode():
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                gy, gmean = kernels.depthwise3x3_blocks_bias_act(x, w, b, act, want_mean=True)
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(2):
            gy.zero_()
            gmean.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(gy, y) and torch.equal(gmean, mean)


# ---- the kernel writes what it owns and nothing else

_PATTERN = {4: (torch.int32, 0x5A5A5A5A), 2: (torch.int16, 0x5A5A)}


def _banded(n, dtype, band=256):
    itype, pattern = _PATTERN[torch.empty(0, dtype=dtype).element_size()]
    whole = torch.full((n + 2 * band,), pattern, device='cuda', dtype=itype)
    inner = whole[band:band + n].view(dtype)
    assert inner.data_ptr() % 16 == 0
    return whole, inner


def _bands_untouched(whole, n, band=256):
    pattern = _PATTERN[whole.element_size()][1]
    return bool((whole[:band] == pattern).all()) and bool((whole[band + n:] == pattern).all())


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,C,H,W', [(7, 1, 12, 12), (1, 7, 4, 4), (70, 3, 12, 12), (3, 3, 6, 8), (1, 5, 28, 44),
                                     (1, 3, 9, 72), (1, 1, 126, 128), (1, 3, 64, 64)])
def test_guard_bands_around_outputs_and_means(B, C, H, W, dtype, hip_lib):
    """Through the C entry, which takes the output pointers: pad lanes, the lanes behind a workgroup's last plane, the
    rows below a partial block row and the planes behind the tensor's end store nothing."""
    from metrabs_amd import _lib, kernels
    x, w, b = _inputs(B, C, H, W, dtype, 700 + H)
    want, want_mean = kernels.depthwise3x3_bias_act(_shifted(x) if kernels.k11_takes_block_kernel(H, W) else x,
                                                    w, b, 'hardswish', 1, 1, want_mean=True)
    n = want.numel()
    wf, bf = w.contiguous().float(), b.contiguous().float()
    for bc in (0, 4, 8) if dtype != F32 and W % 8 == 0 else (0, 4):
        ywhole, y = _banded(n, dtype)
        mwhole, mean = _banded(B * C, F32)
        code = hip_lib.mtr_depthwise3x3_blocks_bias_act_opts(
            x.data_ptr(), _lib.dtype_code(dtype), wf.data_ptr(), bf.data_ptr(), kernels.ACT_CODES['hardswish'], B, C,
            H, W, y.data_ptr(), mean.data_ptr(), _lib.current_stream_ptr(x.device), bc)
        assert code == 0
        torch.cuda.synchronize()
        assert _bands_untouched(ywhole, n) and _bands_untouched(mwhole, B * C), bc
        assert torch.equal(y.view_as(want), want) and torch.equal(mean.view_as(want_mean), want_mean), bc
    ywhole2, y2 = _banded(n, dtype)   # without the mean: the same outputs, nothing else
    code = hip_lib.mtr_depthwise3x3_blocks_bias_act(
        x.data_ptr(), _lib.dtype_code(dtype), wf.data_ptr(), bf.data_ptr(), kernels.ACT_CODES['hardswish'], B, C, H,
        W, y2.data_ptr(), None, _lib.current_stream_ptr(x.device))
    assert code == 0
    torch.cuda.synchronize()
    assert _bands_untouched(ywhole2, n) and torch.equal(y2.view_as(want), want)


# ---- refusals: the entry and the query agree, and nothing is enqueued

def test_refusals_from_the_entry_and_the_query_agree(hip_lib):
    from metrabs_amd import _lib, kernels
    E_SHAPE, E_PARAM, E_ALIGN = -2, -4, -6
    cols = ctypes.c_int(0)
    q = lambda *a: hip_lib.mtr_depthwise3x3_blocks_supported(*a, ctypes.addressof(cols))
    ok = kernels.depthwise3x3_blocks_supported
    # what only the query can be asked (the entry has no stride / padding argument)
    for stride, pad, want in [(2, 1, E_SHAPE), (1, 0, E_SHAPE), (1, (0, 1, 0, 1), E_SHAPE), (1, (0, 2, 1, 1), E_SHAPE),
                              (1, (1, 1, 1, 0), E_SHAPE), (2, (0, 1, 0, 1), E_SHAPE), (3, 1, E_PARAM)]:
        pl, pr, pt, pb = (pad,) * 4 if isinstance(pad, int) else pad
        assert q(0, 12, 12, stride, pt, pl, pb, pr) == want, (stride, pad)
        assert not ok(F32, 12, 12, stride, pad)
    assert q(0, 12, 12, 1, 1, 1, 1, 1) == 0 and ok(F32, 12, 12, 1, 1) and ok(F32, 12, 12)
    sentinel_y = torch.full((2 * 3 * 136 * 136 + 8,), 7.0, device='cuda')
    sentinel_m = torch.full((16,), 7.0, device='cuda')
    st = _lib.current_stream_ptr(sentinel_y.device)
    for H, W, want in [(12, 10, E_SHAPE), (12, 132, E_SHAPE), (132, 12, E_SHAPE), (12, 12, 0), (128, 128, 0),
                       (1, 4, 0), (12, 2, E_SHAPE)]:
        for dtype in DTYPES:
            x, w, b = _inputs(2, 3, H, W, dtype, 1)
            code = hip_lib.mtr_depthwise3x3_blocks_bias_act(
                x.data_ptr(), _lib.dtype_code(dtype), w.data_ptr(), b.data_ptr(), 0, 2, 3, H, W,
                sentinel_y.data_ptr(), sentinel_m.data_ptr(), st) if want else want
            assert code == want, (H, W, dtype)
            assert q(_lib.dtype_code(dtype), H, W, 1, 1, 1, 1, 1) == want
            assert ok(dtype, H, W, 1, 1, x.data_ptr()) == (want == 0)
            if want:
                with pytest.raises(RuntimeError):
                    kernels.depthwise3x3_blocks_bias_act(x, w, b, None)
    # a base off 16 bytes: x, then y
    x, w, b = _inputs(2, 3, 12, 12, F32, 1)
    xs = _shifted(x)
    args = lambda xp, yp: (xp, 0, w.data_ptr(), b.data_ptr(), 0, 2, 3, 12, 12, yp, sentinel_m.data_ptr(), st)
    assert hip_lib.mtr_depthwise3x3_blocks_bias_act(*args(xs.data_ptr(), sentinel_y.data_ptr())) == E_ALIGN
    assert hip_lib.mtr_depthwise3x3_blocks_bias_act(*args(x.data_ptr(), sentinel_y.data_ptr() + 4)) == E_ALIGN
    assert not ok(F32, 12, 12, 1, 1, xs.data_ptr()) and ok(F32, 12, 12, 1, 1, x.data_ptr())
    with pytest.raises(RuntimeError):
        kernels.depthwise3x3_blocks_bias_act(xs, w, b, None)
    # block shapes: 8 columns are a 16-bit shape on rows of whole 16-byte vectors
    opts = hip_lib.mtr_depthwise3x3_blocks_bias_act_opts
    xh = x.half()
    assert opts(*args(x.data_ptr(), sentinel_y.data_ptr()), 8) == E_PARAM
    assert opts(*args(x.data_ptr(), sentinel_y.data_ptr()), 5) == E_PARAM
    assert opts(xh.data_ptr(), 1, w.data_ptr(), b.data_ptr(), 0, 2, 3, 12, 12, sentinel_y.data_ptr(),
                sentinel_m.data_ptr(), st, 8) == E_SHAPE   # W = 12
    assert opts(xh.data_ptr(), 1, w.data_ptr(), b.data_ptr(), 7, 2, 3, 12, 12, sentinel_y.data_ptr(),
                sentinel_m.data_ptr(), st, 0) == E_PARAM   # no such activation
    assert opts(xh.data_ptr(), 3, w.data_ptr(), b.data_ptr(), 0, 2, 3, 12, 12, sentinel_y.data_ptr(),
                sentinel_m.data_ptr(), st, 0) == -3
    assert opts(xh.data_ptr(), 1, w.data_ptr(), b.data_ptr(), 0, 1 << 23, 2, 12, 12, sentinel_y.data_ptr(),
                sentinel_m.data_ptr(), st, 0) == E_SHAPE   # 2^24 planes
    assert opts(None, 1, w.data_ptr(), b.data_ptr(), 0, 2, 3, 12, 12, sentinel_y.data_ptr(),
                sentinel_m.data_ptr(), st, 0) == -1
    with pytest.raises(ValueError):
        kernels.depthwise3x3_blocks_bias_act(x, w, b, None, block_cols=2)
    with pytest.raises(ValueError):
        kernels.depthwise3x3_blocks_bias_act(x.transpose(2, 3), w, b, None)
    with pytest.raises(ValueError):
        kernels.depthwise3x3_blocks_bias_act(x, torch.randn(3, 1, 5, 5, device='cuda'), b, None)
    torch.cuda.synchronize()
    assert bool((sentinel_y == 7.0).all()) and bool((sentinel_m == 7.0).all())   # no refusal enqueued anything


# ---- the armed copies

@functools.lru_cache(maxsize=None)
def _calibrated(name, res):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batches=1, batch_size=2)


def _dw3(net):
    from metrabs_amd import backbones
    return [m for m in net.modules() if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 3]


def _run_recording(net, x):
    """features, [(H, W, stride, has pads, last_path)] of the 3x3 depthwise layers in module order."""
    seen = {}
    hs = [m.register_forward_pre_hook(lambda mod, args: seen.__setitem__(id(mod), tuple(args[0].shape[2:])))
          for m in _dw3(net)]
    try:
        with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            y = net(x)
    finally:
        for h in hs:
            h.remove()
    return y, [(*seen[id(m)], m.stride, m.pads is not None, m.last_path) for m in _dw3(net)]


NETWORKS = [('efficientnetv2-s', 192, 2), ('efficientnetv2-s', 384, 1), ('efficientnetv2-l', 192, 1),
            ('mobilenetv3', 256, 2)]


@pytest.mark.parametrize('dtype', [None, F16, BF16])
@pytest.mark.parametrize('name,res,B', NETWORKS)
def test_armed_copy_runs_k18_with_the_bits_of_the_default_copy(name, res, B, dtype, hip_lib):
    from metrabs_amd import backbones, kernels
    D = backbones.DepthwiseBiasAct
    net = _calibrated(name, res)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, block_depthwise=True)
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in armed.modules()]
    assert not any(m.block_depthwise for m in _dw3(plain))
    assert [m.block_depthwise for m in _dw3(armed)] == [m.stride == 1 and m.pad == 1 and m.pads is None
                                                        for m in _dw3(armed)]
    x = torch.rand(B, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    off, p_off = _run_recording(plain, x)
    on, p_on = _run_recording(armed, x)
    assert torch.isfinite(on).all() and on.dtype == (dtype or F32)
    assert torch.equal(on, off)
    want = [(H, W, s, padded, 'k18' if path == 'k11' and s == 1 and not padded and H <= 128 and W <= 128
             and not kernels.k11_takes_block_kernel(H, W) else path) for H, W, s, padded, path in p_off]
    assert p_on == want
    on_k18 = {(H, W) for H, W, s, padded, path in p_on if path == 'k18'}
    by_plane = lambda paths, hw, s=1: {p[4] for p in paths if p[:2] == hw and p[2] == s}
    # stride 2 keeps its path: K11 (or the library where the output's width is no multiple of 4)
    assert [p for p in p_on if p[2] == 2] == [p for p in p_off if p[2] == 2]
    assert by_plane(p_on, (res // 8, res // 8), 2) == {'k11'}
    if (name, res) == ('efficientnetv2-s', 192):
        assert on_k18 == {(12, 12)} and by_plane(p_on, (6, 6)) == {'library'} == by_plane(p_off, (6, 6))
    elif (name, res) == ('efficientnetv2-s', 384):
        assert on_k18 == {(24, 24), (12, 12)}
    elif name == 'efficientnetv2-l':
        assert on_k18 == {(12, 12)}
    else:
        assert on_k18 == {(128, 128), (64, 64)}
        assert by_plane(p_on, (32, 32)) <= {'k11'} and by_plane(p_on, (16, 16)) <= {'k11'}
        assert by_plane(p_on, (32, 32)) | by_plane(p_on, (16, 16)) == {'k11'}
    # the class switch and a listed shape give the default paths again
    try:
        D.use_k18 = False
        y, p = _run_recording(armed, x)
        assert p == p_off and torch.equal(y, off)
    finally:
        D.use_k18 = True
    layer = next(m for m, p in zip(_dw3(armed), p_on) if p[4] == 'k18')
    C = layer.weight.shape[0]
    H, W = next(p[:2] for m, p in zip(_dw3(armed), p_on) if m is layer)
    try:
        D.k18_slower = frozenset({(C, H, W)})
        y, p = _run_recording(armed, x)
        assert torch.equal(y, off)
        assert [a[4] for a in p] == ['k11' if b[4] == 'k18' and (m.weight.shape[0], b[0], b[1]) == (C, H, W) else b[4]
                                     for m, a, b in zip(_dw3(armed), p, p_on)]
        assert layer.last_path == 'k11'
    finally:
        D.k18_slower = frozenset()
    assert _run_recording(armed, x)[1] == p_on


@pytest.mark.parametrize('dtype', DTYPES)
def test_an_armed_layer_declines_autocast_and_other_layouts(dtype, hip_lib):
    from metrabs_amd import backbones
    net = _calibrated('mobilenetv3', 256)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, block_depthwise=True)
    pairs = [(a, p) for a, p in zip(_dw3(armed), _dw3(plain)) if a.block_depthwise]
    a, p = pairs[0]
    C = a.weight.shape[0]
    x = torch.randn(2, C, 24, 40, device='cuda', generator=torch.Generator(device='cuda').manual_seed(3)).to(dtype)
    with torch.inference_mode():
        want = p(x)
        assert p.last_path == 'k11'
        assert torch.equal(a(x), want) and a.last_path == 'k18'
        with torch.autocast('cuda', dtype=torch.float16):
            assert torch.equal(a(x), p(x)) and a.last_path == 'k11' == p.last_path
        xt = torch.randn(2, C, 40, 24, device='cuda').to(dtype).transpose(2, 3)   # not contiguous
        assert not xt.is_contiguous()
        assert torch.equal(a(xt), p(xt)) and a.last_path == 'library' == p.last_path
        xs = _shifted(x)   # a base off 16 bytes: K11's generic kernel
        assert torch.equal(a(xs), want) and a.last_path == 'k11'
        xo = x[:, :, :, :38].contiguous()   # W % 4 != 0
        assert torch.equal(a(xo), p(xo)) and a.last_path == p.last_path == 'library'
        assert torch.equal(a(x), want) and a.last_path == 'k18'
    if a.emit_mean or any(m.emit_mean for m, _ in pairs):
        a, p = next((m, q) for m, q in pairs if m.emit_mean)
        x = torch.randn(2, a.weight.shape[0], 12, 12, device='cuda').to(dtype)
        with torch.inference_mode():
            ya, yp = a(x), p(x)
            assert a.last_path == 'k18' and torch.equal(ya, yp)
            assert torch.equal(a._mean[1], p._mean[1])


# ---- the loader and the API

def _model_dir(tmp_path):
    from metrabs_amd import backbones, loading
    from metrabs_amd.config import MetrabsConfig
    from metrabs_amd.joint_info import JointInfo
    from metrabs_amd.models.metrabs import Metrabs
    raw = dict(proc_side=192, stride_train=32, stride_test=32, centered_stride=True, depth=8,
               box_size_mm=2200, efficientnet_size='s', weak_perspective=False, mix_3d_inside_fov=0.5)
    bb = backbones.efficientnetv2('s')
    model = Metrabs(bb, JointInfo(cases.COCO17, cases.COCO17_EDGES), MetrabsConfig.from_any(raw),
                    in_channels=bb.out_channels)
    model.load_state_dict(cases.deterministic_state(model.state_dict(), seed=11))
    skel = {'': dict(indices=list(range(17)), names=cases.COCO17, edges=cases.COCO17_EDGES)}
    d = str(tmp_path / 'model')
    loading.save_model_dir(d, model, raw, skel, np.eye(17, dtype=np.float32))
    return d


def _poses(est, images, boxes):
    with torch.inference_mode():
        r = est.estimate_poses_batched(images, boxes, num_aug=2)
    return torch.cat(r['poses3d']).clone()


def test_k18_through_the_loader_and_the_api(tmp_path, hip_lib):
    """A 192 px crop model: its 12x12 depthwise layers are on K18.  Graphed against eager, armed against default."""
    from metrabs_amd import loading
    d = _model_dir(tmp_path)
    ests = {}
    for key, graphed, flag in [('graph', True, True), ('eager', False, True), ('default', False, False)]:
        est = loading.load_multiperson_model(d, dtype=F16, block_depthwise=flag)
        est.crop_model.deterministic_backbone = True
        est.graph_batches = graphed
        ests[key] = est
    images = torch.stack([cases.synth_images(1, 240, 320, 5 + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    for _ in range(2):   # (the second call replays the graph)
        a, b = _poses(ests['eager'], images, boxes), _poses(ests['graph'], images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())
    assert torch.equal(a, _poses(ests['default'], images, boxes))
    for key in ('graph', 'eager'):
        assert 'k18' in {m.last_path for m in _dw3(ests[key].crop_model.backbone)}
    assert 'k18' not in {m.last_path for m in _dw3(ests['default'].crop_model.backbone)}
    st = ests['graph'].graphs.stats
    assert st['captures'] >= 1 and st['replays'] >= 1, st
    f32 = loading.load_crop_model(d, block_depthwise=True)   # dtype=None: an f32 folded copy, armed
    assert any(m.block_depthwise for m in _dw3(f32.backbone))
    assert not any(isinstance(m, torch.nn.BatchNorm2d) for m in f32.backbone.modules())
