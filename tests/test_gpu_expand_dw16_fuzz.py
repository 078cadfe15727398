"""GPU: K25h (csrc/expand_dw16.hip) on shapes drawn from the whole domain it accepts, with the drawing helpers of
tests/conv_fuzz.py: 40 cases from random.Random(a fixed seed), every one inside the domain BY CONSTRUCTION -- Cin from
8 .. 256 in steps of 8, Cmid from 8 .. 400 in steps of 8, the plane from the accepted list (every H, W with H / 4 and
W / 4 powers of two and H W <= 256), B from 1 .. 3, an activation pair, either dtype, the mean wanted or not -- so
nothing is drawn and rejected and no case is skipped: the chain K13h + K11 accepts every one of them too (asserted).
y and the mean must have the chain's bits, and nothing outside them is written."""
import random

import pytest
import torch

import conv_fuzz
from conv_fuzz import ACTS, BF16, F16, _balanced, _bordered, _gen

pytestmark = pytest.mark.gpu

N = 40
PLANES = [(4 << th, 4 << tw) for th in range(5) for tw in range(5) if th + tw <= 4]   # 15 planes, 16 .. 256 positions


def _cases():
    rng = random.Random(2525)
    planes = _balanced(rng, PLANES, N)             # every plane at least twice
    acts1, acts2 = _balanced(rng, ACTS, N), _balanced(rng, ACTS, N)
    dtypes, means = _balanced(rng, [F16, BF16], N), _balanced(rng, [True, True, False], N)
    batches = _balanced(rng, [1, 2, 3], N)
    out = []
    for i in range(N):
        H, W = planes[i]
        out.append(dict(B=batches[i], K=8 * rng.randint(1, 32), M=8 * rng.randint(1, 50), H=H, W=W, act1=acts1[i],
                        act2=acts2[i], dtype=dtypes[i], want_mean=means[i]))
    return out


CASES = _cases()


def _id(c):
    return (f"{c['B']}x{c['K']}-{c['M']}x{c['H']}x{c['W']}-{c['act1']}-{c['act2']}-{str(c['dtype'])[6:]}"
            f"{'-mean' if c['want_mean'] else ''}")


def test_the_draw_covers_the_domain():
    assert len(CASES) == N and len({_id(c) for c in CASES}) == N
    assert {(c['H'], c['W']) for c in CASES} == set(PLANES) and len(PLANES) == 15
    assert {c['dtype'] for c in CASES} == {F16, BF16} and {c['B'] for c in CASES} == {1, 2, 3}
    assert {c['act1'] for c in CASES} == set(ACTS) == {c['act2'] for c in CASES}
    assert any(c['M'] % 64 for c in CASES) and any(c['K'] % 16 for c in CASES) and any(c['K'] > 128 for c in CASES)


@pytest.mark.parametrize('c', CASES, ids=_id)
def test_k25h_fuzz_has_the_chains_bits(c, hip_lib):
    from metrabs_amd import kernels
    B, K, M, H, W, dt = c['B'], c['K'], c['M'], c['H'], c['W'], c['dtype']
    g = _gen('cuda', 1000 + K + M + H)
    x = _bordered(torch.randn(B, K, H, W, device='cuda', generator=g), 8.0).to(dt)
    w1 = (torch.randn(M, K, device='cuda', generator=g) / K ** 0.5).to(dt)
    b1 = 0.5 * torch.randn(M, device='cuda', generator=g)
    wd = torch.randn(M, 1, 3, 3, device='cuda', generator=g) * 0.4
    b2 = torch.randn(M, device='cuda', generator=g)
    # inside the domain of K25h AND of the chain: no case is skipped
    assert hip_lib.mtr_expand_dw16_lds_bytes(B, K, M, H, W) > 0
    assert kernels.expand_depthwise16_supported(x, w1)
    assert kernels.conv1x1_16_supported(x, w1) and kernels.k11_takes_block_kernel(H, W)
    mid = kernels.conv1x1_bias_act16(x, w1, b1, c['act1'])
    want, wmean = kernels.depthwise3x3_bias_act(mid, wd, b2, c['act2'], 1, 1, want_mean=True)
    big, out = conv_fuzz.guarded_out((B, M, H, W), dt, 'cuda')
    got = kernels.expand_depthwise16(x, w1, b1, c['act1'], wd, b2, c['act2'], want_mean=c['want_mean'], out=out)
    y, mean = got if c['want_mean'] else (got, None)
    assert y is out and conv_fuzz.bands_intact(big), 'a write outside out'
    assert torch.equal(y, want), (_id(c), int((y != want).sum()))
    if mean is not None:
        assert torch.equal(mean, wmean), (_id(c), int((mean != wmean).sum()))
