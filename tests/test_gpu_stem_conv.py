"""GPU: K17 (csrc/stem_conv.hip), the backbone stem -- Preproc, the dense 3x3 stride-2 Cin = 3 convolution and the K10
epilogue -- as one launch, through the C-ABI wrapper (kernels.stem_conv_bias_act): against fp64 under a derived
bound, Preproc and the zero ring bit for bit, the same bits for both layouts / any batch index / graph replay, memory
and argument rules, the armed copy of every backbone, the loader and the API.

The bound of `_check`.  With p the tensor K17 convolves (x, or torch's (x * 2 - 1), rounded to `dtype`: the kernel's
own operand bits) and in exact arithmetic z = bias + sum_k w_k p_k, S = |bias| + sum_k |w_k| |p_k|:
  * 16-bit operands: every product w_k p_k is exact in f32 (two 11-bit or 8-bit significands).  The MFMA adds the
    K = 32 slots of its two 16-k steps (27 taps and 5 zero slots, which join the sum) into an f32 accumulator: at most
    K roundings, each of a partial sum of magnitude <= S, each <= 2^-24 S.  f32 operands: an fmaf chain over K = 28
    slots (27 taps and one zero), one rounding per step: the same form with K = 28.
  * the bias addition is one more f32 rounding: (K + 1) 2^-24 S in all, in front of the activation.
  * the activation multiplies an input error by at most its Lipschitz constant L: 1 (none, relu), 1.1 (silu:
    max |silu'| = 1.0998), 1.5 (hardswish: (2 x + 3) / 6 at x = 3).
  * the activation's own roundings: relu none; hardswish rounds x + 3 (<= 2^-24 (|x| + 3), times |x| / 6 inside the
    clamp: <= 2^-24 |z|) and two products and the constant 1 / 6 (<= 4 2^-24 |ref|); silu rounds the exponent's
    argument (relative error |x| 2^-23 of exp(-x), on the result x^2 s (1 - s) 2^-23 <= 0.45 2^-23), v_exp_f32,
    the sum, v_rcp_f32 (1 ulp) and the product: <= 8 2^-24 |ref| + 2^-23.  Both are covered by
    1e-6 |ref| + 2^-24 |z| + 2^-23.
  * one output rounding to `dtype`: half a unit in the last place of the result, taken as one unit of the reference
    (the result may sit in the binade above).
bound = ulp_dtype(ref) + L (K + 1) 2^-24 S + 1e-6 |ref| + 2^-24 |z| + 2^-23.  Every element of every case is compared.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases

pytestmark = pytest.mark.gpu

F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
# (x dtype, dtype of the weight and of y): every pair the entry accepts
PAIRS = [(F32, F32), (F16, F16), (BF16, BF16), (F32, F16), (F32, BF16)]
ACTS = [None, 'relu', 'silu', 'hardswish']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
_LIP = {None: 1.0, 'relu': 1.0, 'silu': 1.1, 'hardswish': 1.5}
_MANT = {F32: 23, F16: 10, BF16: 7}
_CODE = {F32: 0, F16: 1, BF16: 2}
HW = [(8, 8), (2, 8), (24, 40), (64, 64), (130, 136)]
COUTS = [8, 16, 24, 32, 40, 64]
REAL = [(160, 24), (160, 16), (224, 24), (224, 16), (256, 24), (256, 16), (384, 32)]


def _band_rows(Wo):
    """stem_band_rows of stem_conv.hip: the largest power of two <= min(32, 1024 / Wo), at least 1."""
    cap = min(32, max(1, 1024 // Wo))
    th = 1
    while 2 * th <= cap:
        th *= 2
    return th


def test_case_list_holds_every_kind_of_band(hip_lib):
    """The band height recomputed here is the library's: for every map of the case list and every dtype the query
    entry answers the LDS bytes of 3 channels x (2 TH + 1) staged rows of W + 8 elements plus the four waves' 32
    epilogue rows (of 36 f32 or 68 16-bit elements) -- and with that TH the list holds every kind of map."""
    kinds = set()
    for H, W in HW + [(r, r) for r, _ in REAL]:
        Ho, th = H // 2, _band_rows(W // 2)
        kinds.add('smaller' if Ho < th else 'one' if Ho == th else 'plus_one' if Ho % th == 1 else 'many')
        for code, es, ldp in ((0, 4, 36), (1, 2, 68), (2, 2, 68)):
            for M in (8, 24, 64):
                assert hip_lib.mtr_stem_conv_lds_bytes(code, 3, 3, M, H, W) == \
                    (3 * (2 * th + 1) * (W + 8) + 4 * 32 * ldp) * es, (code, M, H, W, th)
    assert {'smaller', 'one', 'plus_one', 'many'} <= kinds, kinds
    assert _band_rows(32) == 32 and 64 // 2 == 32           # 64 x 64: exactly one band
    assert _band_rows(68) == 8 and (130 // 2) % 8 == 1      # 130 x 136: whole bands plus one row
    assert _band_rows(128) == 8 and _band_rows(192) == 4 and _band_rows(4) == 32


def _layout(x, interleaved):
    """The same values over interleaved [B, H, W, 3] memory (a channels_last view) or planar."""
    return x.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) if interleaved else x.contiguous()


def _inputs(B, M, H, W, seed, xdt, dt, border=1.0, unit=False):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.rand(B, 3, H, W, device='cuda', generator=g) if unit else \
        torch.randn(B, 3, H, W, device='cuda', generator=g)
    if border != 1.0:   # large border pixels, a small interior: a wrong ring (a missed or a doubled edge tap) shows
        edge = torch.full((H, W), 0.05, device='cuda')
        edge[0, :] = edge[-1, :] = edge[:, 0] = edge[:, -1] = border
        x = x * edge
    w = (torch.randn(M, 3, 3, 3, device='cuda', generator=g) / 27 ** 0.5).to(dt)
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    return x.to(xdt), w, b


def _torch_p(x, dt, preproc):
    """What the chain feeds its convolution today: torch's own (x * 2 - 1), cast to the copy's dtype."""
    return (x * 2 - 1).to(dt) if preproc else x.to(dt)


def _reference(p, w, b):
    z = F.conv2d(p.double(), w.double(), None, 2, 1) + b.double()[None, :, None, None]
    s = F.conv2d(p.double().abs(), w.double().abs(), None, 2, 1) + b.double().abs()[None, :, None, None]
    return z, s


def _bound(z, s, act, dt):
    """(fp64 result, the bound of the module docstring) from _reference's (z, s)."""
    K = 28 if dt == F32 else 32
    ref = _TORCH_ACT[act](z)
    tiny = torch.finfo(dt).tiny
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(tiny))) - _MANT[dt])
    return ref, ulp + _LIP[act] * (K + 1) * 2.0 ** -24 * s + 1e-6 * ref.abs() + 2.0 ** -24 * z.abs() + 2.0 ** -23


def _check(z, s, act, got, dt, what, worst):
    ref, bound = _bound(z, s, act, dt)
    assert got.shape == ref.shape and got.dtype == dt and got.is_contiguous()
    err = (got.double() - ref).abs()
    share = float((err / bound).max())
    worst[0] = max(worst[0], share)
    assert float((err - bound).max()) <= 0, (what, act, share)


@pytest.mark.parametrize('xdt,dt', PAIRS)
@pytest.mark.parametrize('B', [1, 3])
def test_k17_matches_fp64_on_every_case(B, xdt, dt, hip_lib):
    from metrabs_amd import kernels
    worst, n = [0.0], 0
    for M in COUTS:
        for H, W in HW:
            n += 1
            preproc, inter = bool(n & 1), bool(n & 2)
            x, w, b = _inputs(B, M, H, W, 100 + n, xdt, dt, unit=preproc)
            x = _layout(x, inter)
            assert kernels.stem_conv_supported(x, w), (M, H, W)
            z, s = _reference(_torch_p(x, dt, preproc), w, b)
            for act in ACTS:
                _check(z, s, act, kernels.stem_conv_bias_act(x, w, b, act, preproc=preproc), dt,
                       (B, M, H, W, preproc, inter), worst)
    print(f'k17 fp64 B {B} {xdt} -> {dt}: {n} cases x {len(ACTS)} activations, max err / bound = {worst[0]:.3f}')


@pytest.mark.parametrize('xdt,dt', PAIRS)
def test_k17_matches_fp64_at_the_real_widths(xdt, dt, hip_lib):
    from metrabs_amd import kernels
    worst = [0.0]
    for i, (res, M) in enumerate(REAL):
        x, w, b = _inputs(1, M, res, res, 300 + i, xdt, dt, unit=True)
        x = _layout(x, bool(i & 1))
        z, s = _reference(_torch_p(x, dt, True), w, b)
        for act in ACTS:
            _check(z, s, act, kernels.stem_conv_bias_act(x, w, b, act, preproc=True), dt, (res, M), worst)
    print(f'k17 fp64 real widths {xdt} -> {dt}: max err / bound = {worst[0]:.3f}')


@pytest.mark.parametrize('xdt,dt', PAIRS)
def test_k17_large_border_pixels_small_interior(xdt, dt, hip_lib):
    from metrabs_amd import kernels
    worst = [0.0]
    for i, (H, W) in enumerate([(24, 40), (130, 136), (2, 8)]):
        x, w, b = _inputs(2, 24, H, W, 400 + i, xdt, dt, border=8.0)
        x = _layout(x, bool(i & 1))
        for preproc in (False, True):
            z, s = _reference(_torch_p(x, dt, preproc), w, b)
            for act in (None, 'silu'):
                _check(z, s, act, kernels.stem_conv_bias_act(x, w, b, act, preproc=preproc), dt, (H, W), worst)
    print(f'k17 fp64 borders {xdt} -> {dt}: max err / bound = {worst[0]:.3f}')


@pytest.mark.parametrize('xdt,dt', PAIRS)
def test_k17_rows_that_need_more_than_64k_of_lds(xdt, dt, hip_lib):
    """2 x 4096 (16-bit) and 2 x 2048 (f32): one band is three rows of W + 8 elements, above the default 64 KiB."""
    from metrabs_amd import kernels
    W = 2048 if dt == F32 else 4096
    assert hip_lib.mtr_stem_conv_lds_bytes(_CODE[dt], 1, 3, 16, 2, W) > 64 * 1024
    worst = [0.0]
    x, w, b = _inputs(1, 16, 2, W, 11, xdt, dt, unit=True)
    z, s = _reference(_torch_p(x, dt, True), w, b)
    _check(z, s, 'relu', kernels.stem_conv_bias_act(x, w, b, 'relu', preproc=True), dt, W, worst)


@pytest.mark.parametrize('inter', [False, True])
@pytest.mark.parametrize('xdt,dt', PAIRS)
def test_k17_preproc_has_torchs_bits(xdt, dt, inter, hip_lib):
    """preproc=1 on x against preproc=0 on torch's own (x * 2 - 1).to(dtype): the same bits."""
    from metrabs_amd import kernels
    for i, (H, W, M) in enumerate([(24, 40, 24), (130, 136, 16), (64, 64, 40)]):
        x, w, b = _inputs(2, M, H, W, 500 + i, xdt, dt, unit=(i != 1))   # (i == 1: values outside [0, 1] too)
        x = _layout(x, inter)
        p = _layout(_torch_p(x, dt, True), inter)
        for act in (None, 'hardswish'):
            assert torch.equal(kernels.stem_conv_bias_act(x, w, b, act, preproc=True),
                               kernels.stem_conv_bias_act(p, w, b, act, preproc=False)), (H, W, M, act)


@pytest.mark.parametrize('inter', [False, True])
@pytest.mark.parametrize('xdt,dt', PAIRS)
def test_k17_is_exact_on_small_integers_with_a_zero_ring(xdt, dt, inter, hip_lib):
    """x in {0, 0.5, 1} -> p in {-1, 0, 1}; integer weights without any symmetry in (m, ci, ky, kx), integer bias:
    every partial sum is an integer below 2^8 (bf16's exact range), so the result must be exact.  Image 0 is
    constant x = 0 (p = -1 everywhere): a ring of -1 instead of zero would change every border output."""
    from metrabs_amd import kernels
    for (H, W, M) in [(8, 8, 8), (24, 40, 24), (130, 136, 40)]:
        g = torch.Generator(device='cuda').manual_seed(H)
        x = torch.randint(0, 3, (3, 3, H, W), device='cuda', generator=g).float() / 2
        x[0] = 0
        k = torch.arange(M * 27, device='cuda').view(M, 3, 3, 3)
        m = torch.arange(M, device='cuda').view(M, 1, 1, 1)
        w = ((k * 5 + m * 3 + k // 9) % 7 - 3).float()
        b = (torch.arange(M, device='cuda') % 5 - 2).float()
        p = x * 2 - 1
        ref = F.conv2d(p.double(), w.double(), b.double(), 2, 1)            # padding 1: a ZERO ring around p
        wrong = F.conv2d(F.pad(p.double(), (1, 1, 1, 1), value=-1.0), w.double(), b.double(), 2, 0)
        assert float(ref.abs().max()) <= 27 * 3 + 2 < 2 ** 8 and not torch.equal(ref[0], wrong[0])
        xi = _layout(x.to(xdt), inter)
        for act in (None, 'relu'):
            got = kernels.stem_conv_bias_act(xi, w.to(dt), b, act, preproc=True)
            assert torch.equal(got.double(), _TORCH_ACT[act](ref)), (H, W, M, act)
        got = kernels.stem_conv_bias_act(_layout(p.to(xdt), inter), w.to(dt), b, None, preproc=False)
        assert torch.equal(got.double(), ref)


@pytest.mark.parametrize('xdt,dt', PAIRS)
def test_k17_same_bits_for_layout_batch_call_out_and_graph(xdt, dt, hip_lib):
    from metrabs_amd import kernels
    for (H, W, M) in [(130, 136, 24), (64, 64, 64)]:
        x, w, b = _inputs(3, M, H, W, 7, xdt, dt, unit=True)
        a = kernels.stem_conv_bias_act(x, w, b, 'silu', preproc=True)
        assert torch.equal(a, kernels.stem_conv_bias_act(x, w, b, 'silu', preproc=True))       # call against call
        xi = _layout(x, True)
        assert not xi.is_contiguous()
        assert torch.equal(a, kernels.stem_conv_bias_act(xi, w, b, 'silu', preproc=True))      # planar / interleaved
        for i in range(3):                                                                     # any batch index
            assert torch.equal(a[i:i + 1], kernels.stem_conv_bias_act(x[i:i + 1], w, b, 'silu', preproc=True))
            assert torch.equal(a[i:i + 1], kernels.stem_conv_bias_act(xi[i:i + 1], w, b, 'silu', preproc=True))
        # out= inside guard bands (272 bytes in front, 64 elements behind: y's base stays 16-byte aligned, not
        # 256-byte aligned, whatever the element size)
        g = 272 // a.element_size()
        flat = torch.full((g + a.numel() + 64,), 7.0, device='cuda', dtype=dt)
        out = flat[g:g + a.numel()].view_as(a)
        assert out.data_ptr() % 16 == 0 and out.data_ptr() % 256 != 0
        assert kernels.stem_conv_bias_act(x, w, b, 'silu', preproc=True, out=out) is out
        assert torch.equal(out, a)
        assert bool((flat[:g] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        with torch.inference_mode():
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                kernels.stem_conv_bias_act(xi, w, b, 'silu', preproc=True, out=out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    kernels.stem_conv_bias_act(xi, w, b, 'silu', preproc=True, out=out)
            torch.cuda.current_stream().wait_stream(st)
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, a)
            assert bool((flat[:g] == 7.0).all()) and bool((flat[-64:] == 7.0).all())
        # a shifted, 16-byte-aligned base of x is accepted, one 8 bytes off is refused
        per16 = 16 // x.element_size()
        xflat = torch.zeros(x.numel() + per16, device='cuda', dtype=xdt)
        x16 = xflat[per16:].view_as(x).copy_(x)
        assert x16.data_ptr() % 256 != 0 and kernels.stem_conv_supported(x16, w)
        assert torch.equal(kernels.stem_conv_bias_act(x16, w, b, 'silu', preproc=True), a)
        x8 = xflat[per16 // 2:per16 // 2 + x.numel()].view_as(x)
        assert not kernels.stem_conv_supported(x8, w)
        with pytest.raises(RuntimeError):
            kernels.stem_conv_bias_act(x8, w, b, 'silu')


def test_k17_entry_point_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (the output stays untouched)."""
    from metrabs_amd import kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(1 << 16, device='cuda', dtype=torch.float16)
    sentinel = torch.full((1 << 14,), 7.0, device='cuda', dtype=torch.float16)
    p, q = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(sentinel.data_ptr())
    f = hip_lib.mtr_stem_conv3x3s2

    def call(x=p, xdt=1, layout=0, w=p, b=p, dt=1, act=0, pre=1, B=1, Cin=3, Cout=8, H=8, W=8, y=q):
        return f(x, xdt, layout, w, b, dt, act, pre, B, Cin, Cout, H, W, y, null)

    for name in ('x', 'w', 'b', 'y'):
        assert call(**{name: null}) == -1, name                          # MTR_E_NULL
    assert call(dt=3) == -3 and call(xdt=3) == -3                        # unknown codes
    assert call(xdt=1, dt=2) == -3 and call(xdt=2, dt=1) == -3           # f16 <-> bf16
    assert call(xdt=1, dt=0) == -3 and call(xdt=2, dt=0) == -3           # a 16-bit x into an f32 copy
    assert call(Cin=4) == -2 and call(Cin=1) == -2 and call(Cin=8) == -2
    assert call(H=7) == -2 and call(H=0) == -2
    assert call(W=12) == -2 and call(W=4) == -2 and call(W=0) == -2
    assert call(Cout=12) == -2 and call(Cout=72) == -2 and call(Cout=0) == -2
    assert call(B=-1) == -2 and call(B=65536) == -2
    assert call(act=7) == -4 and call(layout=2) == -4 and call(pre=2) == -4
    assert call(y=p) == -4                                               # y aliases x
    assert call(y=ctypes.c_void_p(t.data_ptr() + 64)) == -4              # y overlaps x
    odd = ctypes.c_void_p(t.data_ptr() + 8)
    assert call(x=odd) == -6 and call(y=ctypes.c_void_p(sentinel.data_ptr() + 8)) == -6   # MTR_E_ALIGN
    assert call(w=ctypes.c_void_p(t.data_ptr() + 1)) == -6 and call(b=ctypes.c_void_p(t.data_ptr() + 2)) == -6
    assert call(B=0) == 0                                                # nothing to do
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())

    x, w, b = _inputs(2, 8, 8, 8, 1, F16, F16)
    ok = kernels.stem_conv_bias_act(x, w, b, None)
    assert ok.shape == (2, 8, 4, 4)
    x4 = torch.zeros(2, 4, 8, 8, device='cuda', dtype=F16)
    with pytest.raises(RuntimeError):
        kernels.stem_conv_bias_act(x4, torch.zeros(8, 4, 3, 3, device='cuda', dtype=F16), b, None)   # Cin != 3
    for bad in (x[:, :, :7], x[:, :, :, :4]):                                                  # odd H, W % 8
        with pytest.raises((RuntimeError, ValueError)):
            kernels.stem_conv_bias_act(bad.contiguous(), w, b, None)
    with pytest.raises(ValueError):
        kernels.stem_conv_bias_act(x[:, :, ::2], w, b, None)                                    # neither layout
    for M in (12, 72):
        wm = torch.zeros(M, 3, 3, 3, device='cuda', dtype=F16)
        assert not kernels.stem_conv_supported(x, wm)
        with pytest.raises(RuntimeError):
            kernels.stem_conv_bias_act(x, wm, torch.zeros(M, device='cuda'), None)
    with pytest.raises(RuntimeError):
        kernels.stem_conv_bias_act(x, w.bfloat16(), b, None)                                    # f16 x, bf16 weight
    with pytest.raises(RuntimeError):
        kernels.stem_conv_bias_act(x, w.float(), b, None)                                       # f16 x, f32 weight
    with pytest.raises(ValueError):
        kernels.stem_conv_bias_act(x, w, b[:4], None)
    with pytest.raises(ValueError):
        kernels.stem_conv_bias_act(x, w, b, None, out=torch.empty(2, 8, 4, 4, device='cuda'))  # out of another dtype
    with pytest.raises(RuntimeError):                                                           # y aliases x
        kernels.stem_conv_bias_act(x, w, b, None, out=x.view(-1)[:2 * 8 * 4 * 4].view(2, 8, 4, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        kernels.stem_conv_bias_act(x.cpu(), w.cpu(), b.cpu(), None)
    assert not kernels.stem_conv_supported(x4, w) and not kernels.stem_conv_supported(x[:, :, ::2], w)
    assert not kernels.stem_conv_supported(x, w.bfloat16()) and not kernels.stem_conv_supported(x, w.float())
    assert kernels.stem_conv_supported(x, w) and kernels.stem_conv_supported(x.float(), w)


def test_k17_shape_query_agrees_with_the_launch(hip_lib):
    """The query's answer against what the entry itself returns (B = 0: its checks without a launch)."""
    t = torch.zeros(64, device='cuda')
    sentinel = torch.full((64,), 7.0, device='cuda')
    p, q, null = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(sentinel.data_ptr()), ctypes.c_void_p(0)
    declined = 0
    for dt in (0, 1, 2):
        for (Cin, Cout, H, W) in [(3, 24, 256, 256), (3, 16, 256, 256), (3, 32, 384, 384), (3, 64, 2, 8),
                                  (3, 24, 255, 256), (3, 24, 256, 252), (3, 20, 64, 64), (3, 72, 64, 64),
                                  (4, 24, 64, 64), (3, 24, 16, 8192), (3, 24, 64, 4096)]:
            n = hip_lib.mtr_stem_conv_lds_bytes(dt, 0, Cin, Cout, H, W)
            assert 0 <= n <= 160 * 1024
            e = hip_lib.mtr_stem_conv3x3s2(p, dt, 0, p, p, dt, 0, 1, 0, Cin, Cout, H, W, q, null)
            assert (e == 0) == (n > 0) and e in (0, -2), (dt, Cin, Cout, H, W, e, n)
            declined += n == 0
    assert hip_lib.mtr_stem_conv_lds_bytes(3, 1, 3, 24, 64, 64) == 0
    assert hip_lib.mtr_stem_conv_lds_bytes(1, 64, 3, 24, 256, 256) == (3 * 17 * 264 + 4 * 32 * 68) * 2
    assert hip_lib.mtr_stem_conv_lds_bytes(0, 64, 3, 24, 256, 256) == (3 * 17 * 264 + 4 * 32 * 36) * 4
    assert declined >= 15
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())


# ---- the armed copy

def _calibrated(name, res, batch_size=4):
    from metrabs_amd import backbones
    torch.manual_seed(0)
    return backbones.calibrate_batchnorm(backbones.build_backbone(name).cuda(), res, 'cuda', batch_size=batch_size)


def _paths(net):
    return [(type(m).__name__, getattr(m, 'last_path', None)) for m in net.modules()]


def _stem_of(net):
    from metrabs_amd import backbones
    pre = [m for m in net.modules() if isinstance(m, backbones.Preproc)]
    stems = [m for m in net.modules() if isinstance(m, backbones.StemConvBiasAct)]
    return pre, stems


@pytest.mark.parametrize('dtype', [F16, BF16, None])
@pytest.mark.parametrize('name', ['efficientnetv2-s', 'efficientnetv2-l', 'mobilenetv3'])
def test_armed_copy_runs_k17_with_the_bits_of_the_default_copy_behind_it(name, dtype, hip_lib):
    from metrabs_amd import backbones, kernels
    S = backbones.StemConvBiasAct
    res = 128
    net = _calibrated(name, res)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    plain2 = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_stem=False)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_stem=True)
    for c in (plain, plain2):   # without the option: nothing armed, nothing new on any module
        pre, stems = _stem_of(c)
        assert not stems and len(pre) == 1 and 'hand_to' not in pre[0].__dict__ and pre[0].hand_to == ()
    assert list(plain.state_dict()) == list(armed.state_dict())
    assert [type(m) for m in plain.modules() if not isinstance(m, backbones.ConvBiasAct)] == \
        [type(m) for m in armed.modules() if not isinstance(m, backbones.ConvBiasAct)]
    (pre,), (stem,) = _stem_of(armed)
    assert pre.hand_to == (stem,) and isinstance(pre.hand_to, tuple)
    plain_stem = next(m for m in plain.modules() if type(m) is backbones.ConvBiasAct and S.applies_to(m.conv))
    wdt = dtype or F32
    assert stem.conv.weight.dtype == wdt and stem.conv.weight.shape[1:] == (3, 3, 3)
    x = torch.rand(3, 3, res, res, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    xs = {'nchw': x, 'channels_last': x.to(memory_format=torch.channels_last)}
    if dtype is not None:
        xs['16-bit channels_last'] = x.to(dtype).to(memory_format=torch.channels_last)
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        ref = net(x).float()
        off = plain(x)
        assert torch.equal(off, plain2(x)) and _paths(plain) == _paths(plain2)
        for what, xin in xs.items():
            on = armed(xin)
            assert stem.last_path == 'k17', what
            assert on.dtype == wdt and on.is_contiguous() and torch.isfinite(on).all()
            # exactness without a tolerance: the default copy with its stem's output replaced by K17's
            y17 = kernels.stem_conv_bias_act(xin, stem.conv.weight, stem.bias, stem.act_name, preproc=True)
            h = plain_stem.register_forward_hook(lambda mod, args, out: y17)
            try:
                swapped = plain(xin)
            finally:
                h.remove()
            assert torch.equal(swapped, on), what
            print(f'{name} {dtype} {what}: mean |copy - f32 net| armed {float((on.float() - ref).abs().mean()):.6g} '
                  f'default {float((off.float() - ref).abs().mean()):.6g} max |f32| {float(ref.abs().max()):.4g}')
        assert not stem.k17_takes(x.cpu()) and not stem.k17_takes(x[:, :, :, ::2])
        # the fallbacks run the chain of the default copy: the same bits, 'library'
        want = plain_stem(x * 2 - 1)
        try:
            S.use_k17 = False
            assert torch.equal(armed(x), plain(x)) and stem.last_path == 'library'
            assert _paths(armed) == [(('StemConvBiasAct', p[1]) if m is plain_stem else p)
                                     for p, m in zip(_paths(plain), plain.modules())]
        finally:
            S.use_k17 = True
        try:
            S.k17_slower = frozenset({(stem.conv.out_channels, res, res)})
            assert torch.equal(stem(pre(x)), want) and stem.last_path == 'library'
        finally:
            S.k17_slower = frozenset()
        with torch.autocast('cuda', dtype=torch.float16):
            got = stem(pre(x))
            assert stem.last_path == 'library'
            assert torch.equal(got, plain_stem(x * 2 - 1))
        odd = x[:, :, :, :res - 4].contiguous()   # W % 8 != 0: a shape K17 does not take
        assert torch.equal(stem(pre(odd)), plain_stem(odd * 2 - 1)) and stem.last_path == 'library'
    was = stem.conv.weight.requires_grad
    with torch.enable_grad():
        stem.conv.weight.requires_grad_(True)
        try:
            assert not stem.k17_takes(x)   # a gradient is wanted
        finally:
            stem.conv.weight.requires_grad_(was)


@pytest.mark.parametrize('cond', ['switch_off', 'listed', 'autocast', 'gradient'])
@pytest.mark.parametrize('dtype', [F16, None])
def test_a_tensor_handed_over_on_the_gpu_and_then_declined_is_still_preprocessed(dtype, cond, hip_lib):
    """Preproc says yes on a CUDA tensor and hands it over untouched; before the stem runs, the condition flips.  The
    stem then applies x * 2 - 1 itself and runs the chain of the default copy: the same bits, 'library'."""
    from metrabs_amd import backbones
    S = backbones.StemConvBiasAct
    net = _calibrated('mobilenetv3', 64)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype)
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=dtype, fuse_stem=True)
    (pre,), (stem,) = _stem_of(armed)
    plain_stem = next(m for m in plain.modules() if type(m) is backbones.ConvBiasAct and S.applies_to(m.conv))
    x = torch.rand(2, 3, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(2))
    was = stem.conv.weight.requires_grad
    try:
        with torch.no_grad(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
            handed = pre(x)
            assert handed is x and stem._handed is x   # a real hand-over: the tensor is still raw
            if cond == 'switch_off':
                S.use_k17 = False
            elif cond == 'listed':
                S.k17_slower = frozenset({(16, 64, 64)})
            elif cond == 'gradient':
                stem.conv.weight.requires_grad_(True)
            with torch.autocast('cuda', dtype=torch.float16, enabled=cond == 'autocast'), \
                    torch.set_grad_enabled(cond == 'gradient'):
                assert not stem.k17_takes(handed)
                got = stem(handed)
                want = plain_stem(x * 2 - 1)
            assert stem.last_path == 'library' and stem._handed is None
            assert torch.equal(got.detach(), want)
            # and not the convolution of the raw tensor
            with torch.autocast('cuda', dtype=torch.float16, enabled=cond == 'autocast'):
                assert not torch.equal(got.detach(), plain_stem(x))
    finally:
        S.use_k17, S.k17_slower = True, frozenset()
        stem.conv.weight.requires_grad_(was)
    with torch.no_grad():   # afterwards the armed copy is back on K17
        stem(pre(x))
        assert stem.last_path == 'k17'


def test_resnet18_arms_nothing(hip_lib):
    from metrabs_amd import backbones
    net = _calibrated('resnet18', 128)
    plain = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=F16)
    opt = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=F16, fuse_stem=True)
    assert _stem_of(opt) == ([], [])
    assert list(plain.state_dict()) == list(opt.state_dict())
    assert [type(m) for m in plain.modules()] == [type(m) for m in opt.modules()]
    x = torch.rand(2, 3, 128, 128, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        assert torch.equal(plain(x), opt(x))
    assert _paths(plain) == _paths(opt)


_FRESH = r'''
import sys, torch
sys.path.insert(0, sys.argv[1])
from metrabs_amd import backbones
net = backbones.build_backbone('mobilenetv3')
net.load_state_dict(torch.load(sys.argv[3]))
net = net.cuda().eval()
copy = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=torch.float16)
x = torch.rand(2, 3, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
    y = copy(x)
torch.save(dict(y=y.cpu(), keys=list(copy.state_dict()), types=[type(m).__name__ for m in copy.modules()],
                paths=[getattr(m, 'last_path', None) for m in copy.modules()]), sys.argv[2])
'''


def test_default_copy_is_that_of_a_process_that_never_used_the_flag(tmp_path, hip_lib):
    """The default copy, folded and run AFTER fuse_stem has been used here, against the same copy folded in a fresh
    process in which the flag was never passed: same module types, keys, paths and bits."""
    from conftest import ROOT
    from metrabs_amd import backbones
    out, state = str(tmp_path / 'fresh.pt'), str(tmp_path / 'state.pt')
    net = _calibrated('mobilenetv3', 64)
    torch.save(net.state_dict(), state)
    subprocess.run([sys.executable, '-c', _FRESH, ROOT, out, state], check=True, timeout=300,
                   env=dict(os.environ, PYTHONPATH=os.pathsep.join(sys.path)))
    fresh = torch.load(out)
    x = torch.rand(2, 3, 64, 64, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1))
    armed = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=F16, fuse_stem=True)
    with torch.inference_mode(), torch.backends.cudnn.flags(enabled=True, benchmark=False, deterministic=True):
        armed(x)
        assert _stem_of(armed)[1][0].last_path == 'k17'
        copy = backbones.fold_batchnorm(net, fused_epilogue=True, dtype=F16)
        y = copy(x)
    assert list(copy.state_dict()) == fresh['keys']
    assert [type(m).__name__ for m in copy.modules()] == fresh['types']
    assert [getattr(m, 'last_path', None) for m in copy.modules()] == fresh['paths']
    assert torch.equal(y.cpu(), fresh['y'])


# ---- the loader and the API

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


def _poses(est, images, boxes):
    with torch.inference_mode():
        r = est.estimate_poses_batched(images, boxes, num_aug=2)
    return torch.cat(r['poses3d']).clone()


def test_k17_through_the_loader_and_the_api(tmp_path, hip_lib):
    from metrabs_amd import backbones, loading
    d = _model_dir(tmp_path)
    est = loading.load_multiperson_model(d, dtype=F16, fuse_stem=True)
    est.crop_model.deterministic_backbone = True
    est.graph_batches = True
    eager = loading.load_multiperson_model(d, dtype=F16, fuse_stem=True)
    eager.crop_model.deterministic_backbone = True
    eager.graph_batches = False
    images = torch.stack([cases.synth_images(1, 240, 320, 5 + i)[0] for i in range(2)]).cuda()
    boxes = [torch.tensor([[60.0, 20.0, 120.0, 200.0], [150.0, 30.0, 100.0, 180.0]]),
             torch.tensor([[40.0, 10.0, 140.0, 210.0]])]
    for _ in range(2):   # (the second call replays the graph)
        a, b = _poses(eager, images, boxes), _poses(est, images, boxes)
        assert torch.isfinite(a).all()
        assert torch.equal(a, b), float((a - b).abs().max())   # a graphed call returns the eager call's bits
    for model in (est, eager):
        assert _stem_of(model.crop_model.backbone)[1][0].last_path == 'k17'
    assert est.graphs.stats['captures'] >= 1 and est.graphs.stats['replays'] >= 1, est.graphs.stats
    f32 = loading.load_crop_model(d, fuse_stem=True)   # dtype=None: the f32 copy gets the f32 kernel
    (stem,) = _stem_of(f32.backbone)[1]
    assert stem.conv.weight.dtype == F32

    # predict_multi: interleaved f16 crops, read in place by K17; the rest of the copy runs its own kernels
    def own_kernel_paths(model):
        return [m.last_path for m in model.backbone.modules()
                if isinstance(m, (backbones.ConvBiasAct, backbones.Conv3x3BiasAct))]

    image = torch.rand(4, 256, 256, 3, generator=cases.gen(5)).half().cuda()
    K = cases.intrinsics_for(256, 256, 40.0)[None].repeat(4, 1, 1).cuda()
    nchw = image.permute(0, 3, 1, 2).contiguous()
    unarmed = loading.load_crop_model(d, dtype=F16).cuda()
    unarmed.deterministic_backbone = True
    armed = eager.crop_model
    with torch.inference_mode():
        for model, closes_the_gap in ((armed, True), (unarmed, False)):
            p_nchw = model.forward((nchw, K))
            on_nchw = own_kernel_paths(model)
            assert any(p in ('k13h', 'k14h') for p in on_nchw)
            p_multi = model.predict_multi(image, K)
            on_multi = own_kernel_paths(model)
            assert p_multi.shape == (4, 17, 3) and torch.isfinite(p_multi).all()
            lost = [i for i, (a, b) in enumerate(zip(on_nchw, on_multi)) if b == 'library' and a != 'library']
            if closes_the_gap:
                assert torch.equal(p_multi, p_nchw) and not lost and on_multi == on_nchw
            else:   # the gap K17 closes: behind the library stem's channels_last activation K13h / K14h decline
                assert lost
