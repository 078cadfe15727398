"""GPU: K13h's deep-K configuration (csrc/conv1x1_16.hip, mtr_conv1x1_bias_act16_opts config 2) against fp64 and,
bit for bit, against the other configurations: on the smallest shapes at which its ring, its tails and its tiles can go
wrong, on three real project classes, for every epilogue; untouched inputs and guard bands; determinism and graph
replays; the argument rules of the two new entries; shifted bases; the default of the Python wrapper.

The design as built: workgroup tile BM x BN = 64 x 64 (2 x 2 waves of one 32 x 32 MFMA tile), k-tiles of BK = 64 in
a ring of S = 3 LDS stages (two more tiles in flight in registers); the unguarded main loop runs from 6 k-tiles on."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BM, BN, BK, S = 64, 64, 64, 3
DTYPES = [torch.float16, torch.bfloat16]
ACTS = [None, 'relu', 'silu', 'hardswish']
CONFIGS = ['deepk', 'tall', 'square', 'auto']
_TORCH_ACT = {None: lambda t: t, 'relu': F.relu, 'silu': F.silu, 'hardswish': F.hardswish}
_MANT = {torch.float16: 10, torch.bfloat16: 7}
GUARD = 64   # elements in front of and behind `out` (a multiple of 8: the output stays 16-byte aligned)

# fewer k-tiles than ring stages (8, BK); k tails (BK + 8, S BK - 8); exactly S tiles and S tiles + 8; the first trip
# before the unguarded main loop (5 tiles), through it once with an even and an odd tile count and a tail (6 BK,
# 7 BK - 8), and twice (8 BK + 8)
KS = [8, BK, BK + 8, S * BK - 8, S * BK, S * BK + 8, 5 * BK, 6 * BK, 7 * BK - 8, 8 * BK + 8]
# below one 32-row tile, not a multiple of 32, past one workgroup
MS = [8, 40, BM + 8]
# (H, W): H W = 8, 16, 24 under BN -- columns past B HW, tiles spanning images (B = 3: 24, 48 and 72 columns; 72 is a
# second workgroup with a tail); B = 1 with M <= BM is a one-workgroup launch
HWS = [(2, 4), (4, 4), (4, 6)]
BS = [1, 3]


def _inputs(B, K, M, H, W, seed, gate, residual, dtype):
    g = torch.Generator(device='cuda').manual_seed(seed)
    x = torch.randn(B, K, H, W, device='cuda', generator=g).to(dtype)
    w = (torch.randn(M, K, 1, 1, device='cuda', generator=g) / K ** 0.5).to(dtype)
    b = 0.5 * torch.randn(M, device='cuda', generator=g)
    gt = torch.rand(B, K, device='cuda', generator=g) if gate else None
    r = torch.randn(B, M, H, W, device='cuda', generator=g).to(dtype) if residual else None
    return x, w, b, gt, r


def _check(x, w, b, act, gt, r, got):
    """|got - fp64| <= one unit in the last place of the 16-bit result + an f32-accumulation term
    1.1 K 2^-24 sum_k |w xg| (through the activation, Lipschitz <= 1.1 here) + 1e-6 |ref| + 2^-24, where xg is
    torch's x * gate.to(x.dtype) and the fp64 sum runs over the 16-bit operands."""
    dt = x.dtype
    xg = x if gt is None else x * gt.to(dt)[:, :, None, None]
    wd = w.double().flatten(1)
    K = x.shape[1]
    z = torch.einsum('mk,bkhw->bmhw', wd, xg.double()) + b.double()[None, :, None, None]
    s = torch.einsum('mk,bkhw->bmhw', wd.abs(), xg.double().abs()) + b.double().abs()[None, :, None, None]
    ref = _TORCH_ACT[act](z)
    if r is not None:
        ref = ref + r.double()
    tiny = torch.finfo(dt).tiny
    ulp = torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(tiny))) - _MANT[dt])
    bound = ulp + 1.1 * K * 2.0 ** -24 * s + 1e-6 * ref.abs() + 2.0 ** -24
    assert got.shape == ref.shape and got.dtype == dt
    excess = float(((got.double() - ref).abs() - bound).max())
    assert excess <= 0, excess


def _guarded(B, M, H, W, dtype):
    n = B * M * H * W
    buf = torch.full((n + 2 * GUARD,), -777.0, device='cuda', dtype=dtype)
    return buf, buf[GUARD:GUARD + n].view(B, M, H, W)


def _one_case(B, K, M, H, W, seed, act, gate, residual, dtype):
    """Everything a case checks; returns nothing."""
    from metrabs_amd import kernels
    x, w, b, gt, r = _inputs(B, K, M, H, W, seed, gate, residual, dtype)
    kept = [t.clone() for t in (x, w, b, gt, r) if t is not None]
    buf, out = _guarded(B, M, H, W, dtype)
    got = kernels.conv1x1_bias_act16(x, w, b, act, gate=gt, residual=r, out=out, config='deepk')
    assert got is out
    ctx = (B, K, M, H, W, act, gate, residual)
    _check(x, w, b, act, gt, r, got)
    assert bool((buf[:GUARD] == -777.0).all()) and bool((buf[-GUARD:] == -777.0).all()), ctx
    for cfg in CONFIGS[1:]:
        assert torch.equal(got, kernels.conv1x1_bias_act16(x, w, b, act, gate=gt, residual=r, config=cfg)), (cfg, ctx)
    if gate:   # the gate rounding rule: the staged x * g has exactly the bits of torch's x * g.to(x.dtype)
        pre = x * gt.to(dtype)[:, :, None, None]
        assert torch.equal(got, kernels.conv1x1_bias_act16(pre, w, b, act, residual=r, config='deepk')), ctx
    for t, k in zip([t for t in (x, w, b, gt, r) if t is not None], kept):
        assert torch.equal(t, k), ctx


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('gate', [False, True])
@pytest.mark.parametrize('residual', [False, True])
def test_deepk_on_the_smallest_shapes_where_it_can_go_wrong(residual, gate, act, dtype, hip_lib):
    from metrabs_amd import kernels
    assert kernels.conv1x1_16_plan(8, 8, 8, 1, 'deepk') == ('deepk', BM // 32, BM, BN)
    seed = 0
    for K in KS:
        for M in MS:
            for H, W in HWS:
                for B in BS:
                    seed += 1
                    _one_case(B, K, M, H, W, seed, act, gate, residual, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
@pytest.mark.parametrize('shape', [(2, 2304, 384, 12, 12), (2, 1536, 256, 8, 8), (1, 3840, 640, 12, 12)])
def test_deepk_on_real_project_classes(shape, act, dtype, hip_lib):
    for i, (gate, residual) in enumerate([(False, False), (True, False), (False, True), (True, True)]):
        _one_case(*shape, 100 + i, act, gate, residual, dtype)


@pytest.mark.parametrize('dtype', DTYPES)
def test_deepk_is_deterministic_and_graph_safe(dtype, hip_lib):
    from metrabs_amd import kernels
    for shape in [(3, 8 * BK + 8, BM + 8, 4, 6), (2, 1536, 256, 8, 8)]:
        x, w, b, gt, r = _inputs(*shape, 3, True, True, dtype)
        run = lambda out=None: kernels.conv1x1_bias_act16(x, w, b, 'silu', gate=gt, residual=r, out=out,
                                                          config='deepk')
        a = run()
        assert torch.equal(a, run())
        with torch.inference_mode():
            out = torch.empty_like(a)
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                run(out)
                st.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                    run(out)
            torch.cuda.current_stream().wait_stream(st)
            for _ in range(2):
                out.zero_()
                graph.replay()
                torch.cuda.synchronize()
                assert torch.equal(out, a)


def test_entry_point_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (the output stays untouched)."""
    null = ctypes.c_void_p(0)
    t = torch.zeros(1024, device='cuda', dtype=torch.float16)
    sentinel = torch.full((512,), 7.0, device='cuda', dtype=torch.float16)
    p = ctypes.c_void_p(t.data_ptr())
    q = ctypes.c_void_p(sentinel.data_ptr())
    odd = ctypes.c_void_p(t.data_ptr() + 8)
    f = hip_lib.mtr_conv1x1_bias_act16_opts
    for cfg in (-1, 0, 1, 2):
        assert f(null, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -1     # MTR_E_NULL
        assert f(p, 1, null, p, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -1
        assert f(p, 1, p, null, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -1
        assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, null, null, cfg) == -1
        assert f(p, 0, p, p, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -3        # f32: K13's entry
        assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 36, q, null, cfg) == -2        # H*W = 36: not a multiple of 8
        assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 49, q, null, cfg) == -2
        assert f(p, 1, p, p, null, null, 0, 1, 8, 12, 16, q, null, cfg) == -2       # Cin = 12
        assert f(p, 1, p, p, null, null, 7, 1, 8, 8, 16, q, null, cfg) == -4        # act code
        assert f(p, 2, p, p, null, null, 0, 1, 8, 8, 16, p, null, cfg) == -4        # y aliases x
        assert f(p, 2, p, p, null, p, 0, 1, 8, 8, 16, q, null, cfg) == -4           # residual aliases x
        assert f(odd, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -6      # misaligned x, weight, y, residual
        assert f(p, 1, odd, p, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -6
        assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, odd, null, cfg) == -6
        assert f(p, 1, p, p, null, odd, 0, 1, 8, 8, 16, q, null, cfg) == -6
        assert f(p, 1, p, p, null, null, 0, 0, 8, 8, 16, q, null, cfg) == 0         # B = 0: nothing to do
    for cfg in (-2, 3, 7):
        assert f(p, 1, p, p, null, null, 0, 1, 8, 8, 16, q, null, cfg) == -4        # no such configuration
    plan = (ctypes.c_int * 4)(7, 7, 7, 7)
    g = hip_lib.mtr_conv1x1_plan16
    assert g(8, 8, 16, 1, 2, null) == -1
    assert g(8, 8, 16, 1, 3, ctypes.addressof(plan)) == -4 and list(plan) == [7, 7, 7, 7]
    assert g(8, 8, 16, 1, 2, ctypes.addressof(plan)) == 0 and list(plan) == [2, BM // 32, BM, BN]
    torch.cuda.synchronize()
    assert bool((sentinel == 7.0).all())
    from metrabs_amd import kernels
    x, w, b, _, _ = _inputs(1, 8, 8, 4, 4, 1, False, False, torch.float16)
    with pytest.raises(KeyError):
        kernels.conv1x1_bias_act16(x, w, b, None, config='wide')


@pytest.mark.parametrize('dtype', DTYPES)
def test_shifted_bases_and_the_default_config(dtype, hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W = 3, BK + 8, 40, 4, 6
    x, w, b, gt, r = _inputs(B, K, M, H, W, 9, True, True, dtype)
    want = kernels.conv1x1_bias_act16(x, w, b, 'relu', gate=gt, residual=r, config='deepk')
    # without `config`: the library's own choice, the call of before
    assert torch.equal(kernels.conv1x1_bias_act16(x, w, b, 'relu', gate=gt, residual=r), want)
    assert torch.equal(kernels.conv1x1_bias_act16(x, w, b, 'relu', gate=gt, residual=r, config='auto'), want)

    def shifted(t, by=8):   # the same values at a base 16 bytes further on
        buf = torch.zeros(t.numel() + 2 * by, device='cuda', dtype=t.dtype)
        buf[by:by + t.numel()] = t.flatten()
        v = buf[by:by + t.numel()].view(t.shape)
        assert v.data_ptr() % 16 == 0 and v.data_ptr() % 32 != t.data_ptr() % 32 and v.is_contiguous()
        return v

    xs, ws, rs, gs, bs = shifted(x), shifted(w), shifted(r), shifted(gt, 4), shifted(b, 4)
    buf, out = _guarded(B, M, H, W, dtype)
    out8 = buf[GUARD + 8:GUARD + 8 + out.numel()].view(out.shape)
    got = kernels.conv1x1_bias_act16(xs, ws, bs, 'relu', gate=gs, residual=rs, out=out8, config='deepk')
    assert torch.equal(got, want)
    assert bool((buf[:GUARD + 8] == -777.0).all()) and bool((buf[GUARD + 8 + out.numel():] == -777.0).all())
