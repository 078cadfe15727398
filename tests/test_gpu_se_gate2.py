"""GPU: K12 after its rewrite (csrc/se.hip: 16 waves per workgroup, the transposed fc2 weight, forcible workgroup
splits) against an fp64 torch evaluation under a bound derived from the two f32 sums; that an image's gate does not
depend on B, on its slot in a workgroup, on the layout of W2 or on the split; guard bands, repeat calls, graph replay
and the argument checks of mtr_se_gate_opts."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

# one-lane channel count, S not a multiple of the 4 rows of a wave, C / 4 past one 64-lane pass by one vector, the
# bench's stage 6, EfficientNetV2-L's last stage (two load rounds per row, ten row blocks per wave)
SHAPES = [(8, 2), (72, 18), (260, 5), (1536, 64), (3840, 160)]
BATCHES = [1, 3, 5, 64]   # ragged last image group for every split (2, 4, 8 images), and more groups than one
PAIRS = [('silu', 'sigmoid'), ('relu', 'hardsigmoid'), ('silu', 'hardsigmoid'), ('relu', 'sigmoid')]
CONFIGS = [0, 1, 2, 3]
U = 2.0 ** -24            # unit roundoff of f32


def _inputs(B, C, S, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    mean = torch.randn(B, C, device='cuda', generator=g)
    w1 = torch.randn(S, C, 1, 1, device='cuda', generator=g) / C ** 0.5
    b1 = 0.1 * torch.randn(S, device='cuda', generator=g)
    w2 = torch.randn(C, S, 1, 1, device='cuda', generator=g) / S ** 0.5
    b2 = 0.1 * torch.randn(C, device='cuda', generator=g)
    return mean, w1, b1, w2, b2


def _fp64_and_bound(mean, w1, b1, w2, b2, act, gate):
    """The gate in fp64 and a bound on |f32 - fp64| for ANY summation order of the two f32 sums:
      pre = b1 + W1 m:  n additions of exactly rounded-once fma terms, n = C + 1:  <= (C + 2) u (|W1| |m| + |b1|)
      hid = act(pre):   the error of pre through the activation (Lipschitz: SiLU <= 1.1, ReLU 1), plus SiLU's own
                        evaluation x * rcp(1 + exp(-x)) -- exp2 of an argument rounded at |x| log2(e) u, 2 ulp of the
                        hardware exp, one add, one 1-ulp rcp, one product: <= (8 + 2 |x|) u relative
      z = b2 + W2 hid:  |W2| err(hid), plus (S + 2) u (|W2| |hid| + |b2|)
      g = gate_fn(z):   err(z) through the gate (Lipschitz: sigmoid 1/4, hardsigmoid 1/6) plus <= 8 u of its own
                        evaluation (exp, add, division / add, clamp, division; g <= 1)."""
    d = lambda t: t.double()
    C, S = mean.shape[1], b1.shape[0]
    W1, W2 = d(w1).flatten(1), d(w2).flatten(1)
    pre = d(mean) @ W1.T + d(b1)
    e_pre = (C + 2) * U * (d(mean).abs() @ W1.abs().T + d(b1).abs())
    if act == 'silu':
        hid = F.silu(pre)
        e_hid = 1.1 * e_pre + (8 + 2 * pre.abs()) * U * hid.abs()
    else:
        hid = F.relu(pre)
        e_hid = e_pre
    z = hid @ W2.T + d(b2)
    e_z = e_hid @ W2.abs().T + (S + 2) * U * (hid.abs() @ W2.abs().T + d(b2).abs())
    if gate == 'sigmoid':
        return torch.sigmoid(z), e_z / 4 + 8 * U
    return F.hardsigmoid(z), e_z / 6 + 8 * U


@pytest.mark.parametrize('act,gate', PAIRS)
@pytest.mark.parametrize('B', BATCHES)
@pytest.mark.parametrize('C,S', SHAPES)
def test_se_gate_matches_fp64_within_the_derived_bound_for_every_layout_and_split(C, S, B, act, gate, hip_lib):
    from metrabs_amd import kernels
    args = _inputs(B, C, S, 31 * C + B)
    ref, bound = _fp64_and_bound(*args, act, gate)
    got = kernels.se_gate(*args, act, gate)
    assert got.shape == (B, C) and got.dtype == torch.float32
    excess = float(((got.double() - ref).abs() - bound).max())
    print(f'C {C} S {S} B {B} {act}/{gate}: max err {float((got.double() - ref).abs().max()):.3e}, '
          f'max bound {float(bound.max()):.3e}, excess {excess:.3e}')
    assert excess <= 0, excess
    # the transposed weight and every forced split: the same summation order, so the same bits
    w2t = args[3].flatten(1).t().contiguous()
    for config in [-1] + CONFIGS:
        for t in (None, w2t):
            assert torch.equal(kernels.se_gate(*args, act, gate, w2t=t, config=config), got), (config, t is None)


@pytest.mark.parametrize('C,S', SHAPES)
def test_an_images_gate_does_not_depend_on_the_batch_or_its_slot(C, S, hip_lib):
    from metrabs_amd import kernels
    args = _inputs(64, C, S, 5)
    w2t = args[3].flatten(1).t().contiguous()
    full = kernels.se_gate(*args, 'silu', 'sigmoid', w2t=w2t)
    alone = torch.cat([kernels.se_gate(args[0][i:i + 1], *args[1:], 'silu', 'sigmoid', w2t=w2t) for i in range(64)])
    assert torch.equal(full, alone)
    # the same images at other slots of a workgroup (a batch shifted by one, by three)
    for shift in (1, 3):
        part = kernels.se_gate(args[0][shift:].contiguous(), *args[1:], 'silu', 'sigmoid', w2t=w2t)
        assert torch.equal(part, full[shift:])


@pytest.mark.parametrize('config', [-1] + CONFIGS)
@pytest.mark.parametrize('C,S,B', [(260, 5, 5), (1536, 64, 64)])
def test_se_gate_writes_only_its_output_and_repeats_itself(C, S, B, config, hip_lib):
    """Guard bands around `out`, call against call, and a captured graph's replay."""
    from metrabs_amd import kernels
    args = _inputs(B, C, S, 11)
    w2t = args[3].flatten(1).t().contiguous()
    G = 1024
    big = torch.full((B * C + 2 * G,), -7.0, device='cuda')
    out = big[G:G + B * C].view(B, C)
    a = kernels.se_gate(*args, 'relu', 'hardsigmoid', w2t=w2t, config=config)
    kernels.se_gate(*args, 'relu', 'hardsigmoid', w2t=w2t, config=config, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, a)
    assert bool((big[:G] == -7.0).all()) and bool((big[G + B * C:] == -7.0).all())
    with torch.inference_mode():
        st = torch.cuda.Stream()
        st.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(st):
            kernels.se_gate(*args, 'relu', 'hardsigmoid', w2t=w2t, config=config, out=out)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=st, capture_error_mode='thread_local'):
                kernels.se_gate(*args, 'relu', 'hardsigmoid', w2t=w2t, config=config, out=out)
        torch.cuda.current_stream().wait_stream(st)
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, a)
    assert bool((big[:G] == -7.0).all()) and bool((big[G + B * C:] == -7.0).all())


def test_se_gate_opts_argument_checks(hip_lib):
    """No GPU work: every call below is refused before a launch (or has nothing to do)."""
    from metrabs_amd import _lib, kernels
    null = ctypes.c_void_p(0)
    t = torch.zeros(64, device='cuda')
    p = ctypes.c_void_p(t.data_ptr())
    f = hip_lib.mtr_se_gate_opts
    assert _lib.SIGNATURES['mtr_se_gate_opts']
    assert f(null, p, p, p, p, 2, 0, 1, 8, 2, p, null, 0, -1) == -1      # MTR_E_NULL
    assert f(p, p, p, null, p, 2, 0, 1, 8, 2, p, null, 1, -1) == -1
    assert f(p, p, p, p, p, 2, 0, 1, 8, 2, null, null, 0, -1) == -1
    assert f(p, p, p, p, p, 2, 0, 1, 6, 2, p, null, 1, 0) == -2          # C % 4 != 0
    assert f(p, p, p, p, p, 2, 0, 1, 0, 2, p, null, 1, 0) == -2
    assert f(p, p, p, p, p, 2, 0, 1, 8, 0, p, null, 1, 0) == -2
    assert f(p, p, p, p, p, 2, 0, 1, 40960, 64, p, null, 0, -1) == -2    # four mean rows past 160 KiB of LDS
    assert f(p, p, p, p, p, 2, 0, 1, 8192, 64, p, null, 0, 2) == -2      # fits four images, not the eight of split 2
    assert f(p, p, p, p, p, 2, 0, 200000, 8, 2, p, null, 0, 3) == -2     # more than 65535 groups of two images
    assert f(ctypes.c_void_p(t.data_ptr() + 4), p, p, p, p, 2, 0, 1, 8, 2, p, null, 0, -1) == -6   # MTR_E_ALIGN
    assert f(p, ctypes.c_void_p(t.data_ptr() + 8), p, p, p, 2, 0, 1, 8, 2, p, null, 0, -1) == -6
    assert f(p, p, p, p, p, 2, 5, 1, 8, 2, p, null, 0, -1) == -4         # gate code
    assert f(p, p, p, p, p, 9, 0, 1, 8, 2, p, null, 0, -1) == -4         # act code
    assert f(p, p, p, p, p, 2, 0, 1, 8, 2, p, null, 2, -1) == -4         # layout of w2
    assert f(p, p, p, p, p, 2, 0, 1, 8, 2, p, null, 0, 4) == -4          # split
    assert f(p, p, p, p, p, 2, 0, 1, 8, 2, p, null, 0, -2) == -4
    assert f(p, p, p, p, p, 2, 0, 0, 8, 2, p, null, 1, 3) == 0           # B = 0: nothing to do
    args = _inputs(2, 8, 2, 1)
    with pytest.raises(ValueError):
        kernels.se_gate(*args, 'silu', 'sigmoid', w2t=args[3].flatten(1))   # [C, S], not [S, C]


def test_squeeze_excite_hands_over_the_transposed_weight_and_follows_the_weight(hip_lib):
    from metrabs_amd import backbones, kernels
    torch.manual_seed(3)
    se = backbones.SqueezeExcite(72, 18).cuda().eval()
    seen = []
    orig = kernels.se_gate

    def spying(*a, **k):
        seen.append(k.get('w2t'))
        return orig(*a, **k)

    class Src:
        def take_mean_f32(self, x):
            return x.mean((2, 3))

    se.mean_from = (Src(),)
    x = torch.randn(3, 72, 8, 8, device='cuda')
    kernels.se_gate = spying
    try:
        with torch.no_grad():
            a = se(x)
            b = se(x)
            se.fc2.weight.mul_(2.0)
            c = se(x)
    finally:
        kernels.se_gate = orig
    assert len(seen) == 3 and all(t is not None and t.shape == (18, 72) for t in seen)
    assert seen[0] is seen[1] and torch.equal(a, b)
    assert torch.equal(seen[2], se.fc2.weight.flatten(1).t())   # made again after the weight was written
    with torch.no_grad():
        se.mean_from = ()
        ref = se(x)
    assert float((c - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
