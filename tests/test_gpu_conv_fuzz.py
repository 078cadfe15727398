"""GPU: the backbone convolution kernels (K10 .. K22) on shapes DRAWN from the domain their entry points accept
(tests/conv_fuzz.py: 24 seeded cases per kernel, all inside the domain by construction; tests/test_conv_fuzz_host.py
holds the generators to that and to the places the draws must reach).  One parametrized test per kernel, the ids are
the case numbers.  Every case, through metrabs_amd.kernels:

  * the fp64 bound OF THE KERNEL'S OWN TEST MODULE (its `_check`, imported through the adapter; no tolerance of this
    file's own);
  * bit equality where the project promises it: every K13 / K13h configuration that resolves to itself against 'auto';
    a prologue (in_bias, in_act) of K13 and K20 against the same kernel on K10's output; K16h against its two-kernel
    chain wherever the chain's own kernels take the intermediate; K11 / K15 / K18 with and without the mean; K18's
    block shapes and K11's generic kernel; a second call;
  * guard bands: `out` (and the mean) inside a buffer filled with a sentinel, x and the residual inside buffers filled
    with NaN: the bands keep their bits, every element of `out` is written, no NaN reaches it, the inputs are
    untouched.  (kernels.depthwise*_bias_act allocate y themselves: their guarded launch goes through the C entry on
    the same tensors and must give the wrapper's bits.)

Then, per kernel, a handful of cases just outside the domain, one rule broken at a time: the predicate says False, the
C entry returns its documented code, and nothing of a sentinel-filled arena is written."""
import types

import pytest
import torch

import conv_fuzz
from conv_fuzz import GUARD, KERNELS, N_CASES, SENTINEL

pytestmark = pytest.mark.gpu
CASES = list(range(N_CASES))


def _setup(name, i):
    from metrabs_amd import kernels
    k = KERNELS[name]
    c = k.cases()[i]
    inp = k.inputs(c, 'cuda', guard=True, seed=i)
    kept = {n: inp[n].clone() for n in ('x', 'r') if '_big_' + n in inp}
    return kernels, k, c, inp, kept


def _inputs_untouched(inp, kept):
    for n, before in kept.items():
        big = inp['_big_' + n]
        assert torch.equal(inp[n], before), n
        assert bool(torch.isnan(big[:GUARD]).all()) and bool(torch.isnan(big[-GUARD:]).all()), n


def _written_inside(big, out):
    assert conv_fuzz.bands_intact(big), 'a write outside out'
    assert not bool(torch.isnan(out.float()).any()), 'a read outside x or the residual'
    assert not bool((out == SENTINEL).any()), 'an element of out was not written'


def _guarded(kernels, k, c, inp, kept, dtype=None, **kw):
    """The launch with out= carved out of a sentinel-filled buffer -> out, after the guard-band assertions."""
    big, out = conv_fuzz.guarded_out(k.out_shape(c), dtype or c['dtype'], 'cuda')
    assert k.run(kernels, c, inp, out=out, **kw) is out
    _written_inside(big, out)
    _inputs_untouched(inp, kept)
    return out


def _conv1x1(name, i):
    kernels, k, c, inp, kept = _setup(name, i)
    assert k.supported(c, 'cuda') in (None, True)
    out = _guarded(kernels, k, c, inp, kept)
    if inp['b_in'] is not None:   # the bound is on the GEMM's input: K10's result on x
        inp['x10'] = k.gemm_input(c, inp, kernels)
    k.check(c, inp, out)
    assert torch.equal(k.run(kernels, c, inp), out)          # a second call, another out
    if inp['b_in'] is not None:   # the prologue has the bits of K10, then the same kernel
        assert torch.equal(k.run(kernels, c, inp, prologue=False), out)
    return kernels, k, c, inp, kept, out


@pytest.mark.parametrize('i', CASES)
def test_k13(i, hip_lib):
    kernels, k, c, inp, kept, out = _conv1x1('k13', i)
    for config in k.configs(kernels, c)[1:]:
        assert torch.equal(_guarded(kernels, k, c, inp, kept, config=config), out), config


@pytest.mark.parametrize('i', CASES)
def test_k13h(i, hip_lib):
    kernels, k, c, inp, kept, out = _conv1x1('k13h', i)
    for config in k.configs(kernels, c)[1:]:
        assert torch.equal(_guarded(kernels, k, c, inp, kept, config=config), out), config


@pytest.mark.parametrize('i', CASES)
def test_k20(i, hip_lib):
    _conv1x1('k20', i)


def _dense(name, i, dtype=None):
    kernels, k, c, inp, kept = _setup(name, i)
    out = _guarded(kernels, k, c, inp, kept, dtype=dtype)
    k.check(c, inp, out)
    assert torch.equal(k.run(kernels, c, inp), out)
    return kernels, k, c, inp, out


@pytest.mark.parametrize('i', CASES)
def test_k14h(i, hip_lib):
    _dense('k14h', i)


@pytest.mark.parametrize('i', CASES)
def test_k19(i, hip_lib):
    _dense('k19', i)


@pytest.mark.parametrize('i', CASES)
def test_k22(i, hip_lib):
    _dense('k22', i)


@pytest.mark.parametrize('i', CASES)
def test_k16h(i, hip_lib):
    kernels, k, c, inp, out = _dense('k16h', i)
    if c['chain']:   # Ho * Wo % 8 == 0: K13h takes the intermediate, the chain exists
        assert torch.equal(k.run(kernels, c, inp, chain=True), out)


@pytest.mark.parametrize('i', CASES)
def test_k17(i, hip_lib):
    kernels, k, c, inp, out = _dense('k17', i)
    # the same bits from the other layout
    other = dict(inp, x=inp['x'].contiguous() if c['interleaved'] else
                 inp['x'].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2))
    assert torch.equal(k.run(kernels, c, other), out)


def _depthwise(name, i, hip_lib):
    kernels, k, c, inp, kept = _setup(name, i)
    assert k.supported(c, 'cuda') in (None, True)
    got = k.run(kernels, c, inp)
    y, mean = got if c['want_mean'] else (got, None)
    k.check(c, inp, y, mean)
    # the other of (with, without) the mean: the same y
    other = k.run(kernels, dict(c, want_mean=not c['want_mean']), inp)
    assert torch.equal(other if c['want_mean'] else other[0], y)
    # the C entry on the same tensors, y and the mean inside sentinel-filled buffers
    big, out = conv_fuzz.guarded_out(tuple(y.shape), c['dtype'], 'cuda')
    mbig, mout = conv_fuzz.guarded_out((c['B'], c['C']), torch.float32, 'cuda')
    w, b = inp['w'].contiguous().float(), inp['b'].contiguous().float()
    p = types.SimpleNamespace(X=inp['x'].data_ptr(), W=w.data_ptr(), B=b.data_ptr(), Y=out.data_ptr(), M=mout.data_ptr())
    assert k.accept(hip_lib, c, B=c['B'], p=p)[0] == 0
    torch.cuda.synchronize()
    _written_inside(big, out)
    assert torch.equal(out, y)
    assert conv_fuzz.bands_intact(mbig)
    if c['want_mean']:
        assert torch.equal(mout, mean)
    else:
        assert bool((mout == SENTINEL).all())
    _inputs_untouched(inp, kept)
    return kernels, k, c, inp, y, mean


@pytest.mark.parametrize('i', CASES)
def test_k11(i, hip_lib):
    _depthwise('k11', i, hip_lib)


@pytest.mark.parametrize('i', CASES)
def test_k15(i, hip_lib):
    _depthwise('k15', i, hip_lib)


@pytest.mark.parametrize('i', CASES)
def test_k18(i, hip_lib):
    kernels, k, c, inp, y, mean = _depthwise('k18', i, hip_lib)
    # the bits do not depend on the block shape, and they are those of K11's generic kernel (which a base one element
    # further reaches on the planes K11's block kernel would take: tests/test_gpu_depthwise3x3.py)
    shapes = [None, 4] + ([8] if c['dtype'] != torch.float32 and c['W'] % 8 == 0 else [])
    for cols in shapes:
        assert torch.equal(kernels.depthwise3x3_blocks_bias_act(inp['x'], inp['w'], inp['b'], c['act'], block_cols=cols), y)
    x = inp['x']
    if kernels.k11_takes_block_kernel(c['H'], c['W']):
        x = torch.zeros(x.numel() + 8, device='cuda', dtype=x.dtype)[1:1 + x.numel()].view_as(x)
        x.copy_(inp['x'])
    ky, kmean = kernels.depthwise3x3_bias_act(x, inp['w'], inp['b'], c['act'], 1, 1, want_mean=True)
    assert torch.equal(ky, y)
    if mean is not None:
        assert torch.equal(kmean, mean)


@pytest.mark.parametrize('i', CASES)
def test_k10(i, hip_lib):
    """In place: the tensor itself lies between the sentinel bands."""
    kernels, k, c, inp, kept = _setup('k10', i)
    big, work = conv_fuzz._carve(inp['x'], SENTINEL)
    got = k.run(kernels, c, inp, out=work)
    y, mean = got if c['want_mean'] else (got, None)
    assert y.data_ptr() == work.data_ptr()
    assert conv_fuzz.bands_intact(big) and not bool(torch.isnan(y.float()).any())
    k.check(c, inp, y, mean)
    _inputs_untouched(inp, kept)
    again = inp['x'].clone()
    got2 = k.run(kernels, c, inp, out=again)
    assert torch.equal(got2[0] if c['want_mean'] else got2, y)
    if c['want_mean']:
        assert torch.equal(got2[1], mean)


@pytest.mark.parametrize('i', CASES)
def test_se_gate(i, hip_lib):
    kernels, k, c, inp, kept = _setup('se_gate', i)
    out = _guarded(kernels, k, c, inp, kept)
    k.check(c, inp, out)
    assert torch.equal(k.run(kernels, c, inp), out)
    # the layout of W2 and the workgroup split do not change the bits
    assert torch.equal(k.run(kernels, dict(c, w2t=not c['w2t'], config=-1), inp), out)


OUTSIDE = [(name, j) for name, (_, broken) in conv_fuzz.OUTSIDE.items() for j in range(len(broken))]


@pytest.mark.parametrize('name,j', OUTSIDE, ids=[f'{n}-{conv_fuzz.OUTSIDE[n][1][j][0].replace(" ", "_")}' for n, j in OUTSIDE])
def test_one_rule_broken_is_refused_and_nothing_is_written(name, j, hip_lib):
    k = KERNELS[name]
    base, broken = conv_fuzz.OUTSIDE[name]
    what, changed, shift_x, shift_y, code = broken[j]
    c = dict(base, **changed)
    spacing = 1 << 16   # bytes between the arguments: more than any tensor of these cases
    arena = torch.full((len(conv_fuzz.Pointers.NAMES) * spacing // 4,), SENTINEL, device='cuda')
    p = conv_fuzz.Pointers(arena.data_ptr(), spacing)
    assert all(rc == 0 for rc in k.accept(hip_lib, base, B=0, p=p)), 'the case itself is accepted'
    assert k.supported(base, 'cuda') in (None, True)
    p.X += shift_x
    p.Y += shift_y
    assert k.accept(hip_lib, c, B=c['B'], p=p)[0] == code, (name, what)
    # (the predicates look at x and the weights: the output is allocated by the wrapper.  depthwise5x5_supported states
    # the LDS rule alone; the width rule and the stride are DepthwiseBiasAct.path's and applies_to's)
    if shift_y == 0 and (name != 'k15' or 'padded plane' in what):
        assert k.supported(c, 'cuda', shift=shift_x) in (None, False), (name, what)
    torch.cuda.synchronize()
    assert bool((arena == SENTINEL).all()), (name, what)
