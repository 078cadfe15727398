"""GPU: K11 (csrc/depthwise.hip, kernels.depthwise3x3_bias_act) -- depthwise 3x3 + bias + activation (+ the plane
mean) in one pass -- against fp64 on every path of its launcher, exactly on integers, path against path, call
against call and graph replay bit for bit, with guard bands around what it writes, and inside fold_batchnorm.

The accuracy bound (no free tolerance).  Inputs are rounded to the tensor's dtype first, weights and bias are
f32, so every product x*w the kernel forms has the fp64 reference's operands.  With u = 2^-24:
  * pre-activation v: nine fma and the bias.  The generic kernel adds the bias last (10 f32 roundings), the
    stride-1 block kernel seeds the accumulator with it (9 roundings); every partial sum is at most
    S = sum |x*w| + |b| in magnitude: |v_hat - v| <= gamma_10 S < 11 u S (Higham, Accuracy and Stability, eq. 3.7
    applied to the fma chain);
  * the activation (common.h activate<>, the code K15 runs: tests/test_gpu_depthwise5x5.py) is Lipschitz with
    constant L <= 1.5 (hardswish: (2x + 3) / 6 at x = 3; silu 1.1, relu and none 1), which carries that error to
    1.5 * 11 u S, and is itself evaluated in f32: hardswish is an addition, a clamp, two products and the rounded
    constant 1/6 (5 roundings); silu is x * rcp(1 + exp2(-x log2 e)), where the rounded argument of exp2 costs
    2 |v| u relative and v_exp_f32, the addition, v_rcp_f32 (1 ulp = 2 u each) and the product 6 u more: together at
    most (8 + 2 |v|) u |act(v)|;
  * one rounding to the output dtype: u_out |y_hat| with u_out = 2^-24 (f32), 2^-11 (f16), 2^-8 (bf16), plus half
    the smallest subnormal for f16 (2^-25).
  bound = E (1 + u_out) + u_out |act(v)| + tiny,   E = 1.5 * 11 u S + (8 + 2 |v|) u |act(v)|
  * the mean is the f32 sum of the n = OH * OW STORED outputs (n - 1 additions in whatever order) times the rounded
    1 / n: |mean_hat - mean(y)| <= (n + 1) u mean |y|.
The fp64 reference is nine shifted strided slices of the zero-padded input times w[c, ky, kx] plus the bias --
elementwise, so it stays fast at 300 k planes -- pinned once against F.conv2d in fp64.  Each test prints the largest
observed error as a share of this bound.

Which kernel a case reaches is computed by _route, a restatement of launch_depthwise's geometry, and asserted:
a retune that reroutes a case fails test_the_case_list_reaches_every_path instead of silently testing something
else."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _leave_the_device_idle():
    """Nothing of a test here outlives it on the GPU (captured graphs, side streams, the large stepping cases)."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()
    torch.cuda.synchronize()


DTYPES = [torch.float32, torch.float16, torch.bfloat16]
ACTS = [None, 'relu', 'silu', 'hardswish']
U = 2.0 ** -24
U_OUT = {torch.float32: 2.0 ** -24, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}
TINY = {torch.float32: 2.0 ** -126, torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -126}


def _pads(pad):
    return (pad,) * 4 if isinstance(pad, int) else tuple(pad)   # (left, right, top, bottom)


# ---- launch_depthwise's geometry, restated

def _ilog2_exact(v):
    return v.bit_length() - 1 if v > 0 and v & (v - 1) == 0 else -1


def _route(n_planes, H, W, stride, pad, aligned=True):
    """The kernel a launch takes and what its waves walk: dict(path, lanes (per plane), chunks, n_pg, n_waves,
    items (the set of items per wave over the launch's waves), ragged (a partly dead last workgroup / group))."""
    pl, pr, pt, pb = _pads(pad)
    OH, OW = (H + pt + pb - 3) // stride + 1, (W + pl + pr - 3) // stride + 1
    assert OW % 4 == 0 and OH > 0
    symmetric = pl == pr == pt == pb
    if stride == 1:
        tw, th = _ilog2_exact(W // 4), _ilog2_exact(H // 4)
        if symmetric and pt == 1 and W % 4 == 0 and H % 4 == 0 and 0 <= tw <= 4 and th >= 0 and tw + th <= 6 \
                and aligned and n_planes < 2 ** 24:
            lanes = 1 << (tw + th)
            return dict(path='block', lanes=lanes, tw=tw, th=th, chunks=1, n_pg=0, n_waves=0, items={1},
                        ragged=(n_planes * lanes) % 256 != 0)
    groups = OH * (OW // 4)
    lpp = 1
    while lpp < 64 and lpp < groups:
        lpp *= 2
    chunks = (groups + 63) // 64
    ppi = 64 // lpp
    n_pg = (n_planes + ppi - 1) // ppi
    n_waves = 4 * min((n_pg + 3) // 4, 1024)
    if stride == 1:
        vec = W % 4 == 0 and aligned and symmetric and pt == 1
    else:
        vec = W % 4 == 0 and aligned and OW * 2 == W and pl <= 1
    n_min, n_max = (n_pg - min(n_pg, n_waves)) // n_waves + 1, (n_pg + n_waves - 1) // n_waves
    return dict(path=('vec' if vec else 'scalar') + str(stride), lanes=lpp, chunks=chunks, n_pg=n_pg,
                n_waves=n_waves, items={n * chunks for n in range(n_min, n_max + 1)},
                ragged=n_planes % ppi != 0 or groups % 64 != 0, last_chunk=groups - 64 * (chunks - 1))


# ---- the cases: (B, C, H, W, stride, pad (an int or (left, right, top, bottom)), the path they are meant for)

_S2_PADS = [1, (0, 1, 0, 1), (0, 2, 0, 2), (1, 0, 1, 0)]
BLOCK = [
    (2, 3, 4, 4, 1, 1, 'block'),       # one lane per plane: no left / right neighbour
    (1, 1, 4, 4, 1, 1, 'block'), (1, 7, 4, 4, 1, 1, 'block'),
    (2, 3, 4, 8, 1, 1, 'block'), (2, 3, 8, 4, 1, 1, 'block'),
    (2, 3, 8, 8, 1, 1, 'block'), (1, 1, 8, 8, 1, 1, 'block'), (1, 7, 8, 8, 1, 1, 'block'),
    (70, 3, 8, 8, 1, 1, 'block'),      # several plane rows in a DPP row; the last workgroup partly dead
    (2, 3, 16, 16, 1, 1, 'block'), (1, 7, 16, 16, 1, 1, 'block'), (2, 3, 32, 32, 1, 1, 'block'),
    (1, 5, 16, 64, 1, 1, 'block'),     # a plane row fills a whole 16-lane DPP row
    (1, 5, 64, 4, 1, 1, 'block'),      # a one-lane-wide plane
]
VEC1 = [
    (2, 3, 12, 12, 1, 1, 'vec1'),      # W / 4 is no power of two; chunks = 1
    (3, 3, 6, 8, 1, 1, 'vec1'), (2, 3, 10, 16, 1, 1, 'vec1'),   # H % 4 != 0; 6x8: four planes per wave
    (2, 3, 20, 28, 1, 1, 'vec1'), (2, 3, 24, 40, 1, 1, 'vec1'), (1, 5, 28, 44, 1, 1, 'vec1'),   # chunks 3, 4, 5, ragged
    (1, 5, 32, 48, 1, 1, 'vec1'), (1, 5, 28, 64, 1, 1, 'vec1'),   # chunks 6, 7
    (1, 3, 64, 64, 1, 1, 'vec1'),      # chunks = 16
]
VEC2 = [(B, C, H, W, 2, pad, 'vec2') for pad in _S2_PADS
        for B, C, H, W in [(3, 7, 8, 8), (2, 3, 16, 16), (2, 3, 32, 32), (1, 5, 48, 24), (2, 3, 12, 24)]]
SCALAR = [
    (2, 3, 6, 10, 1, 0, 'scalar1'), (2, 3, 10, 18, 1, 0, 'scalar1'),
    (2, 3, 8, 8, 1, (0, 2, 1, 1), 'scalar1'), (2, 3, 12, 24, 1, (0, 2, 1, 1), 'scalar1'),
    (2, 3, 9, 17, 2, 0, 'scalar2'), (3, 7, 6, 10, 2, 0, 'scalar2'),
]
# the 19 cases K11 was tested with before this file (in test_gpu_bias_act.py, where they keep their ids)
EARLIER = [
    (2, 960, 16, 16, 1, 1, 'block'), (3, 256, 32, 32, 2, 1, 'vec2'), (2, 96, 18, 18, 2, 0, 'scalar2'),
    (5, 1536, 8, 8, 1, 1, 'block'), (1, 7, 4, 8, 1, 1, 'block'), (2, 5, 9, 9, 2, 0, 'scalar2'),
    (70, 3, 16, 16, 1, 1, 'block'), (3, 4, 32, 32, 1, 1, 'block'), (2, 5, 64, 64, 2, 1, 'vec2'),
    (2, 6, 10, 18, 1, 0, 'scalar1'), (64, 960, 16, 16, 1, 1, 'block'), (33, 130, 8, 8, 1, 1, 'block'),
    (2, 3, 24, 40, 1, 1, 'vec1'),
    (3, 960, 16, 16, 2, (0, 2, 0, 2), 'vec2'), (2, 256, 32, 32, 2, (0, 1, 0, 1), 'vec2'),
    (2, 7, 8, 24, 2, (1, 0, 1, 0), 'vec2'), (2, 5, 16, 16, 1, (1, 1, 1, 1), 'block'),
    (2, 6, 14, 12, 1, (0, 2, 1, 1), 'scalar1'), (70, 3, 16, 16, 2, (0, 2, 0, 2), 'vec2'),
]
CASES = BLOCK + VEC1 + VEC2 + SCALAR + EARLIER
# persistent stepping: more than 4,096 plane groups of 16 planes (4x4 outputs), a ragged last group.
# (B, C, H, W, stride, pad, path, items per wave); f32 and one 16-bit dtype, one activation each
STEPPING = [
    (29714, 7, 8, 8, 2, 1, 'vec2', {3, 4}, [(torch.float32, 'hardswish'), (torch.bfloat16, 'relu')]),
    (66239, 5, 6, 6, 1, 0, 'scalar1', {5, 6}, [(torch.float32, 'relu'), (torch.float16, 'hardswish')]),
]


def test_the_case_list_reaches_every_path():
    routes = [(c, _route(c[0] * c[1], *c[2:6])) for c in CASES]
    for c, r in routes:
        assert r['path'] == c[6], (c, r)
        if r['path'] != 'scalar1' and r['path'] != 'scalar2':   # the same shape through a shifted base: scalar rows
            assert _route(c[0] * c[1], *c[2:6], aligned=False)['path'] == 'scalar%d' % c[4], c
    paths = {r['path'] for _, r in routes}
    assert paths == {'block', 'vec1', 'vec2', 'scalar1', 'scalar2'}
    block = [r for _, r in routes if r['path'] == 'block']
    assert {r['lanes'] for r in block} >= {1, 2, 4, 16, 64}
    assert {(r['tw'], r['th']) for r in block} >= {(0, 0), (1, 0), (0, 1), (1, 1), (2, 2), (3, 3), (4, 2), (0, 4)}
    assert any(r['ragged'] for r in block) and any(not r['ragged'] for r in block)
    generic = [r for _, r in routes if r['path'] != 'block']
    items = set().union(*(r['items'] for r in generic))
    assert items >= {1, 2, 3, 4, 5, 6, 7, 16}, items
    assert {r['chunks'] for r in generic} >= {1, 2, 3, 4, 5, 6, 7, 16}
    assert {r['lanes'] for r in generic} >= {2, 4, 8, 16, 32, 64}
    assert any(r['chunks'] == 2 and r['last_chunk'] == 8 for r in generic)   # 48x24 -> 24x12
    for path in ('vec1', 'vec2', 'scalar1', 'scalar2'):
        assert any(r['ragged'] for r in generic if r['path'] == path), path
    # items per wave through scalar rows too: the shifted twins of the vector cases
    shifted = [_route(c[0] * c[1], *c[2:6], aligned=False) for c in CASES if c[6] in ('vec1', 'vec2', 'block')]
    assert set().union(*(r['items'] for r in shifted)) >= {1, 2, 3, 4, 5, 6, 7}
    for B, C, H, W, stride, pad, path, want_items, _ in STEPPING:
        r = _route(B * C, H, W, stride, pad)
        assert r['path'] == path and r['n_pg'] > 4096 and r['n_waves'] == 4096 and r['items'] == want_items, r
        assert r['lanes'] == 4 and (B * C) % 16 != 0


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


def _conv64(x, w, b, stride, pad):
    """fp64: (v, S), v = the convolution plus bias as nine shifted strided slices of the padded input times
    w[c, ky, kx], S = the same on absolute values."""
    xd = F.pad(x.double(), _pads(pad))
    B, C, Hp, Wp = xd.shape
    OH, OW = (Hp - 3) // stride + 1, (Wp - 3) // stride + 1
    wd, bd = w.double().reshape(C, 9), b.double().view(1, C, 1, 1)
    v = bd.expand(B, C, OH, OW).clone()
    S = bd.abs().expand(B, C, OH, OW).clone()
    xa = xd.abs()
    for ky in range(3):
        for kx in range(3):
            ys, xs = slice(ky, ky + stride * (OH - 1) + 1, stride), slice(kx, kx + stride * (OW - 1) + 1, stride)
            wk = wd[:, 3 * ky + kx].view(1, C, 1, 1)
            v.addcmul_(xd[:, :, ys, xs], wk)
            S.addcmul_(xa[:, :, ys, xs], wk.abs())
    return v, S


def test_the_reference_is_the_grouped_convolution():
    """Both are ten fp64 roundings of partial sums of at most S: they agree to 2 gamma_10 S in fp64 (exactly, in
    practice)."""
    for stride, pad, H, W in [(1, 1, 5, 8), (2, (0, 1, 0, 1), 6, 8), (1, (0, 2, 1, 1), 4, 6), (2, 0, 7, 9)]:
        x, w, b = _inputs(2, 3, H, W, torch.float32, 11 * H + W, device='cpu')
        v, S = _conv64(x, w, b, stride, pad)
        want = F.conv2d(F.pad(x.double(), _pads(pad)), w.double(), b.double(), stride, 0, groups=3)
        assert v.shape == want.shape
        assert bool(((v - want).abs() <= 22 * 2.0 ** -53 * S).all())


def _ordered(t):
    """The bits of a float tensor as integers in the order of the values (ulp distances are differences)."""
    if t.dtype == torch.float32:
        i = t.contiguous().view(torch.int32).long()
        return torch.where(i < 0, -(i & 0x7fffffff), i)
    i = t.contiguous().view(torch.int16).long()
    return torch.where(i < 0, -(i & 0x7fff), i)


def _bound(v, S, ref, dtype):
    """The bound of the module docstring from the fp64 pre-activation v, S = sum |x w| + |b| and ref = act(v)."""
    E = 1.5 * 11 * U * S + (8 + 2 * v.abs()) * U * ref.abs()
    return E * (1 + U_OUT[dtype]) + U_OUT[dtype] * ref.abs() + TINY[dtype]


def _ref_and_bound(x, w, b, act, stride, pad):
    """(fp64 result, bound) of a whole (small) case: what _check compares every y with (tests/conv_fuzz.py)."""
    v, S = _conv64(x, w, b, stride, pad)
    ref = _act64(v, act)
    return ref, _bound(v, S, ref, x.dtype)


def _check(x, w, b, act, stride, pad, outs, tag='', spread=None):
    """Every (y, mean) of outs against the fp64 bound; the reference is formed once, in slices of the batch of at most
    2^22 outputs (the fp64 temporaries of the largest cases stay small).  Returns the largest shares of the two bounds.
    spread (a dict, with two outs): accumulates how far the two are apart -- outputs that differ, the largest
    difference as a share of the bound, and in ulp where the output is no cancelled sum (|act(v)| >= S / 8: next to
    zero an ulp distance says nothing)."""
    uo, tiny = U_OUT[x.dtype], TINY[x.dtype]
    B = x.shape[0]
    n = outs[0][0][0].numel()
    step = max(1, (1 << 22) // max(1, n))
    share = mshare = 0.0
    for i in range(0, B, step):
        v, S = _conv64(x[i:i + step], w, b, stride, pad)
        ref = _act64(v, act)
        bound = _bound(v, S, ref, x.dtype)
        if spread is not None:
            a, c = outs[0][0][i:i + step], outs[1][0][i:i + step]
            d = (a.double() - c.double()).abs()
            solid = ref.abs() >= S / 8
            spread['n'] = spread.get('n', 0) + d.numel()
            spread['differ'] = spread.get('differ', 0) + int((d > 0).sum())
            spread['share'] = max(spread.get('share', 0.0), float((d / bound).max()))
            spread['ulp'] = max(spread.get('ulp', 0), int(((_ordered(a) - _ordered(c)).abs() * solid).max()))
        del S, v
        for y, mean in outs:
            assert y.shape[1:] == ref.shape[1:] and y.shape[0] == B and y.dtype == x.dtype
            yd = y[i:i + step].double()
            share = max(share, float(((yd - ref).abs() / bound).max()))
            if mean is not None:
                # f32 sum of hw = OH * OW rounded outputs, then one product with the rounded 1 / hw
                hw = y.shape[2] * y.shape[3]
                mbound = (hw + 1) * U * yd.abs().mean((2, 3)) + 2.0 ** -126
                assert mean.shape == y.shape[:2] and mean.dtype == torch.float32
                mshare = max(mshare, float(((mean[i:i + step].double() - yd.mean((2, 3))).abs() / mbound).max()))
    assert share <= 1.0 and mshare <= 1.0, (tag, share, mshare)
    return share, mshare


def _shifted(x):
    """The same tensor at a base one element further: not 16-byte aligned, the launcher's scalar rows."""
    buf = torch.zeros(x.numel() + 8, device=x.device, dtype=x.dtype)
    s = buf[1:1 + x.numel()].view_as(x)
    s.copy_(x)
    assert s.is_contiguous() and s.data_ptr() % 16 != 0
    return s


# ---- every path against fp64

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('act', ACTS)
def test_every_path_matches_fp64(act, dtype, hip_lib):
    """Each case with the mean, without it (same bits), and -- where the aligned base takes vector rows or the block
    kernel -- through a base shifted by one element.  The generic kernel's vector and scalar rows accumulate in one
    order: same bits.  The block kernel seeds its accumulators with the bias where the generic kernel adds it last:
    both inside the bound, the distance between them printed."""
    from metrabs_amd import kernels
    worst, mworst, where, spread = 0.0, 0.0, None, {}
    for i, (B, C, H, W, stride, pad, path) in enumerate(CASES):
        x, w, b = _inputs(B, C, H, W, dtype, 1000 + i)
        assert x.data_ptr() % 16 == 0
        y, mean = kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad, want_mean=True)
        assert torch.equal(y, kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad))
        outs = [(y, mean)]
        if not path.startswith('scalar'):
            outs.append(kernels.depthwise3x3_bias_act(_shifted(x), w, b, act, stride, pad, want_mean=True))
            if path != 'block':
                assert torch.equal(y, outs[1][0]) and torch.equal(mean, outs[1][1]), (i, CASES[i])
        share, mshare = _check(x, w, b, act, stride, pad, outs, tag=CASES[i], spread=spread if path == 'block' else None)
        if share > worst:
            worst, where = share, CASES[i]
        mworst = max(mworst, mshare)
    name = str(dtype)[6:]
    print(f'[k11] paths {name} act={act}: largest share of the bound {worst:.3f} at {where}, of the mean\'s '
          f'summation bound {mworst:.3f}')
    print(f'[k11] paths {name} act={act}: block kernel vs generic kernel (shifted base) on block-eligible shapes: '
          f'{spread["differ"]} of {spread["n"]} outputs differ, by at most {spread["share"]:.3f} of the bound and '
          f'{spread["ulp"]} ulp where |act(v)| >= S / 8')


@pytest.mark.parametrize('B,C,H,W,stride,pad,path,items,runs', STEPPING)
def test_waves_that_step_through_several_plane_groups(B, C, H, W, stride, pad, path, items, runs, hip_lib):
    from metrabs_amd import kernels
    assert len(runs) == 2 and runs[0][0] == torch.float32 and runs[1][0] != torch.float32
    for dtype, act in runs:
        x, w, b = _inputs(B, C, H, W, dtype, B)
        y, mean = kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad, want_mean=True)
        share, mshare = _check(x, w, b, act, stride, pad, [(y, mean)], tag='stepping')
        print(f'[k11] stepping {B * C} planes {path} items per wave {sorted(items)} {str(dtype)[6:]} act={act}: '
              f'largest share of the bound {share:.3f}, of the mean\'s {mshare:.3f}')
        assert torch.equal(y, kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad))
        del x, y, mean


# ---- the shapes the folded backbones run

@functools.lru_cache(maxsize=None)
def _k11_shapes(name, res):
    """(C, H, W, stride, pads, act) of every 3x3 DepthwiseBiasAct of a folded backbone at `res` px."""
    from metrabs_amd import backbones
    net = backbones.fold_batchnorm(backbones.build_backbone(name).eval(), fused_epilogue=True).cuda()
    shapes = set()

    def hook(mod, args):
        x = args[0]
        shapes.add((x.shape[1], x.shape[2], x.shape[3], mod.stride,
                    mod.pads if mod.pads is not None else (mod.pad,) * 4, mod.act_name))

    hs = [m.register_forward_pre_hook(hook) for m in net.modules()
          if isinstance(m, backbones.DepthwiseBiasAct) and m.k == 3]
    with torch.inference_mode():
        for B in (1, 3):
            net(torch.rand(B, 3, res, res, device='cuda'))
    for h in hs:
        h.remove()
    return sorted(shapes, key=str)


# distinct (C, H, W, stride, pads, act) of the 3x3 depthwise layers
WORKLOADS = {('effnetv2-s', 256): 6, ('mobilenetv3', 256): 8, ('effnetv2-l', 384): 7}


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('name,res', sorted(WORKLOADS))
def test_workload_shapes_match_fp64(name, res, dtype, hip_lib):
    from metrabs_amd import kernels
    shapes = _k11_shapes(name, res)
    assert len(shapes) == WORKLOADS[name, res], shapes
    ran, worst, mworst, where = 0, 0.0, 0.0, None
    for i, (C, H, W, stride, pads, act) in enumerate(shapes):
        for B in (1, 3):
            pl, pr, pt, pb = pads
            if B * C * ((H + pt + pb - 3) // stride + 1) * ((W + pl + pr - 3) // stride + 1) > 2 ** 26:
                continue
            x, w, b = _inputs(B, C, H, W, dtype, 2000 + 10 * i + B)
            y, mean = kernels.depthwise3x3_bias_act(x, w, b, act, stride, pads, want_mean=True)
            share, mshare = _check(x, w, b, act, stride, pads, [(y, mean)], tag=(name, shapes[i], B))
            if share > worst:
                worst, where = share, (B,) + shapes[i]
            mworst = max(mworst, mshare)
            ran += 1
    assert ran == 2 * len(shapes)   # nothing at batch 3 comes near 2^26 outputs
    print(f'[k11] {name}@{res} {str(dtype)[6:]}: {ran} launches, largest share of the bound {worst:.3f} at {where}, '
          f'of the mean\'s {mworst:.3f}')


# ---- exactly on integers

_TAPS = (3.0 * (torch.arange(9, dtype=torch.float32) - 4.0)).view(1, 1, 3, 3)   # different at every tap, asymmetric
_EXACT_SHAPES = [(4, 4), (8, 8), (16, 16), (12, 24), (48, 24), (6, 10), (9, 17)]
_EXACT_PADS = [(1, 1), (2, 1), (2, (0, 1, 0, 1)), (2, (0, 2, 0, 2)), (2, (1, 0, 1, 0)), (1, 0), (1, (0, 2, 1, 1)), (2, 0)]


def _exact_case(B, C, H, W, seed):
    """Integers in -1 .. 1 inside the plane and in -2 .. 2 on its border rows and columns, taps -12 .. 12 in steps of
    3 with the sign flipped on every other channel, an integer bias: every product, partial sum and output is a small
    integer, exact in f32, and -- checked by the caller on the CPU -- at most 256, so exact in bf16 too."""
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
    ran = 0
    for H, W in _EXACT_SHAPES:
        x, w, b = _exact_case(3, 6, H, W, 7 * H + W)
        for stride, pad in _EXACT_PADS:
            want = F.conv2d(F.pad(x.double(), _pads(pad)), w.double(), b.double(), stride, 0, groups=6)
            if want.shape[3] % 4:
                continue
            assert 32 <= float(want.abs().max()) <= 256   # exact in bf16, and not trivial
            assert torch.equal(want, want.round())
            y, mean = kernels.depthwise3x3_bias_act(x.cuda().to(dtype), w.cuda(), b.cuda(), None, stride, pad,
                                                    want_mean=True)
            assert torch.equal(y.double().cpu(), want), (H, W, stride, pad, float((y.double().cpu() - want).abs().max()))
            # integer sums below 2^24 are exact in f32; the product with the rounded 1 / n is two roundings
            mwant = want.mean((2, 3))
            assert bool(((mean.double().cpu() - mwant).abs() <= (2 * U + U * U) * mwant.abs()).all()), (H, W, stride, pad)
            ran += 1
    assert ran == 31, ran   # of the 56 combinations, those with OW % 4 == 0


# ---- call against call, graph replay

@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,C,H,W,stride,pad,path,act', [
    (70, 3, 8, 8, 1, 1, 'block', 'silu'), (2, 5, 24, 40, 1, 1, 'vec1', 'hardswish'),
    (3, 7, 48, 24, 2, (0, 1, 0, 1), 'vec2', 'relu'), (3, 5, 10, 18, 1, 0, 'scalar1', None)])
def test_call_against_call_and_graph_replay(B, C, H, W, stride, pad, path, act, dtype, hip_lib):
    from metrabs_amd import kernels
    r = _route(B * C, H, W, stride, pad)
    assert r['path'] == path and (path != 'vec1' or r['chunks'] > 1)
    x, w, b = _inputs(B, C, H, W, dtype, 500 + C)
    y, mean = kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad, want_mean=True)
    _check(x, w, b, act, stride, pad, [(y, mean)], tag='graph')
    y3, mean3 = kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad, want_mean=True)
    assert torch.equal(y, y3) and torch.equal(mean, mean3)
    with torch.inference_mode():
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad, want_mean=True)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                gy, gmean = kernels.depthwise3x3_bias_act(x, w, b, act, stride, pad, want_mean=True)
        torch.cuda.current_stream().wait_stream(st)
        for _ in range(2):
            gy.zero_()
            gmean.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(gy, y) and torch.equal(gmean, mean)


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
@pytest.mark.parametrize('B,C,H,W,stride,pad,path', [
    (7, 1, 8, 8, 1, 1, 'block'), (1, 7, 4, 4, 1, 1, 'block'), (70, 3, 8, 8, 1, 1, 'block'),
    (3, 3, 6, 8, 1, 1, 'vec1'), (1, 5, 28, 44, 1, 1, 'vec1'), (3, 7, 8, 8, 2, (0, 1, 0, 1), 'vec2'),
    (1, 5, 48, 24, 2, 1, 'vec2'), (3, 7, 6, 10, 2, 0, 'scalar2'), (3, 3, 10, 18, 1, 0, 'scalar1')])
def test_guard_bands_around_outputs_and_means(B, C, H, W, stride, pad, path, dtype, hip_lib):
    """Through the C entry, which takes the output pointers: dead lanes and items recompute the last plane and must
    not store it; one lane per plane group writes the means."""
    from metrabs_amd import _lib, kernels
    r = _route(B * C, H, W, stride, pad)
    assert r['path'] == path and r['ragged']
    x, w, b = _inputs(B, C, H, W, dtype, 700 + H)
    want, want_mean = kernels.depthwise3x3_bias_act(x, w, b, 'hardswish', stride, pad, want_mean=True)
    pl, pr, pt, pb = _pads(pad)
    n = want.numel()
    ywhole, y = _banded(n, dtype)
    mwhole, mean = _banded(B * C, torch.float32)
    wf, bf = w.contiguous().float(), b.contiguous().float()
    code = hip_lib.mtr_depthwise3x3_bias_act_padded(
        x.data_ptr(), _lib.dtype_code(dtype), wf.data_ptr(), bf.data_ptr(), kernels.ACT_CODES['hardswish'], B, C, H, W,
        stride, pt, pl, pb, pr, y.data_ptr(), mean.data_ptr(), _lib.current_stream_ptr(x.device))
    assert code == 0
    torch.cuda.synchronize()
    assert _bands_untouched(ywhole, n) and _bands_untouched(mwhole, B * C)
    assert torch.equal(y.view_as(want), want) and torch.equal(mean.view_as(want_mean), want_mean)
    # without the mean: the same outputs, nothing else
    ywhole2, y2 = _banded(n, dtype)
    code = hip_lib.mtr_depthwise3x3_bias_act_padded(
        x.data_ptr(), _lib.dtype_code(dtype), wf.data_ptr(), bf.data_ptr(), kernels.ACT_CODES['hardswish'], B, C, H, W,
        stride, pt, pl, pb, pr, y2.data_ptr(), None, _lib.current_stream_ptr(x.device))
    assert code == 0
    torch.cuda.synchronize()
    assert _bands_untouched(ywhole2, n) and torch.equal(y2.view_as(want), want)


# ---- the wrapper and fold_batchnorm

def test_wrapper_refuses_a_weight_that_is_not_3x3(hip_lib):
    from metrabs_amd import kernels
    x, w, b = _inputs(1, 4, 16, 16, torch.float32, 1)
    w5 = torch.randn(4, 1, 5, 5, device='cuda')
    with pytest.raises(ValueError):
        kernels.depthwise3x3_bias_act(x, w5, b, None, 1, 1)   # read as w[c * 9 + k] it would give a wrong result
    with pytest.raises(ValueError):
        kernels.depthwise3x3_bias_act(x, w[:3], b, None, 1, 1)
    assert kernels.depthwise3x3_bias_act(x, w.view(4, 3, 3), b, None, 1, 1).shape == x.shape
    with pytest.raises(ValueError):
        kernels.depthwise3x3_bias_act(x.transpose(2, 3), w, b, None, 1, 1)


def test_fold_batchnorm_folds_the_zero_padding_into_k11(hip_lib):
    """The explicit ZeroPad2d of the reference's TF-'SAME' stride-2 layers (efficientnet.py:1127-1161: (0,1,0,1);
    (0,2,0,2) for the bottomright_stride layer) becomes an argument of K11."""
    from metrabs_amd import backbones
    net = backbones.build_backbone('effnetv2-s').eval()
    fused = backbones.fold_batchnorm(net, fused_epilogue=True)
    padded = [m for m in fused.modules() if isinstance(m, backbones.DepthwiseBiasAct) and m.pads is not None]
    assert [m.pads for m in padded] == [(0, 2, 0, 2)]  # the bottomright_stride layer
    n_pad = lambda n: sum(isinstance(m, torch.nn.ZeroPad2d) for m in n.modules())
    assert n_pad(fused) == n_pad(net) - 1
